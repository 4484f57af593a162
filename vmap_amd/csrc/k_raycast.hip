// k_raycast.hip - the TSDF ray cast (raycast_kernels.h): brick classes of a volume, and its depth, status, normal and colour images.
// gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "raycast_kernels.h"

namespace vl {

int tsdf_bricks(int nx, int ny, int nz, float min_weight, const float* tsdf, const float* weight, unsigned char* bricks, hipStream_t st) {
    vray::BricksArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nx = nx; a.ny = ny; a.nz = nz; a.min_weight = min_weight;
    a.tsdf = tsdf; a.weight = weight; a.bricks = bricks;
    const unsigned columns = (unsigned)(rc::brick_dim(nx) * rc::brick_dim(ny));           // <= 128 * 128
    hipLaunchKernelGGL(vray::tsdf_bricks, dim3(columns), dim3(vray::kBricksWG), 0, st, a);
    return launched("tsdf_bricks");
}

int tsdf_raycast(const vmapstep_raycast_cfg& c, const float* tsdf, const float* weight, const float* color, const unsigned char* bricks, int n_bricks,
                 const float* views, int n_views, float* depth, unsigned char* status, float* normal, unsigned char* color_out, hipStream_t st) {
    vray::RaycastArgs a;
    std::memset(&a, 0, sizeof(a));
    rc::Rules& r = a.rules;
    r.fx = c.fx; r.fy = c.fy; r.cx = c.cx; r.cy = c.cy;
    r.min_depth = c.min_depth; r.max_depth = c.max_depth; r.step = c.step; r.min_weight = c.min_weight;
    r.width = c.width; r.height = c.height; r.max_steps = c.max_steps;
    r.nx = c.nx; r.ny = c.ny; r.nz = c.nz;
    std::memcpy(r.N, c.normal_map, sizeof(r.N));
    a.vol.tsdf = tsdf; a.vol.weight = weight; a.vol.color = color;
    a.bricks = bricks; a.n_bricks = n_bricks;
    a.views = views;
    a.depth = depth; a.status = status; a.normal = normal; a.color_out = color_out;
    const long long tiles = ceil_div(c.width, vray::kTile) * ceil_div(c.height, vray::kTile);   // < 2^31 / 12 / 64 + ...: fits the grid
    const unsigned blocks = (unsigned)ceil_div(tiles, vray::kTilesPerWG);
    for (int v0 = 0; v0 < n_views; v0 += vray::kMaxViewsPerLaunch) {
        const int nv = n_views - v0 < vray::kMaxViewsPerLaunch ? n_views - v0 : vray::kMaxViewsPerLaunch;
        a.view0 = v0;
        hipLaunchKernelGGL(vray::tsdf_raycast, dim3(blocks, (unsigned)nv), dim3(vray::kRaycastWG), 0, st, a);
    }
    return launched("tsdf_raycast");
}

}  // namespace vl
