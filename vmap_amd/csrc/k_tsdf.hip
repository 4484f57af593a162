// k_tsdf.hip - TSDF fusion (tsdf_kernels.h): posed depth frames into a truncated signed distance volume and a colour volume.
// gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "tsdf_kernels.h"

namespace vl {

int tsdf_integrate(const vmapstep_tsdf_cfg& c, float* tsdf, float* weight, float* color, const float* depth, const unsigned char* rgbx,
                   const int* inst, const float* t_wc, const int* slots, int n_frames, hipStream_t st) {
    vtsdf::IntegrateArgs a;
    std::memset(&a, 0, sizeof(a));
    cr::Rules& cam = a.rules.cam;
    cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy;
    cam.min_depth = c.min_depth; cam.width = c.width; cam.height = c.height; cam.margin = c.margin;
    a.rules.max_depth = c.max_depth; a.rules.trunc = c.trunc; a.rules.max_weight = c.max_weight; a.rules.obj_id = c.obj_id;
    a.nx = c.nx; a.ny = c.ny; a.nz = c.nz; a.n = c.nx * c.ny * c.nz;
    std::memcpy(a.A, c.affine, sizeof(a.A));
    a.tsdf = tsdf; a.weight = weight; a.color = color;
    a.depth = depth; a.rgbx = color ? rgbx : nullptr; a.inst = c.obj_id >= 0 ? inst : nullptr;
    a.t_wc = t_wc; a.slots = slots; a.n_frames = n_frames;
    const unsigned tiles = (unsigned)ceil_div(a.n, vtsdf::kTsdfTile);
    if (color)
        hipLaunchKernelGGL(vtsdf::tsdf_integrate<true>, dim3(tiles), dim3(vtsdf::kTsdfWG), 0, st, a);
    else
        hipLaunchKernelGGL(vtsdf::tsdf_integrate<false>, dim3(tiles), dim3(vtsdf::kTsdfWG), 0, st, a);
    return launched("tsdf_integrate");
}

}  // namespace vl
