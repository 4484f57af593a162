// raycast_kernels.h - the TSDF ray cast on the device: depth, status, normal and colour images of a truncated signed distance volume
// from any number of poses, with no mesh in between.  The rule is raycast_rules.h's; the contract is the raycast section of
// include/vmapstep.h.
//
//   tsdf_bricks        one class byte per brick of 8 x 8 x 8 cells (rc::BrickClass).  A workgroup owns one (a, b) column of bricks and
//                      a lane one k: the up to 81 rows of the column are read along k, the fast axis, each row's loads contiguous over
//                      the workgroup.  A lane keeps, per row, whether voxels k and k + 1 are both valid (nine bits per i-slab; two
//                      consecutive slabs ANDed give the cells), and whether all it saw was valid and exactly 1.0f; a ballot folds the
//                      eight lanes of a brick, its first lane writes the byte.  The apron voxel a brick shares with its neighbour is
//                      read by both.  No atomics.
//   tsdf_raycast       one lane per pixel, views on grid.y.  A wave is an 8 x 8 pixel tile, h fast within it as in the image: its 64
//                      rays walk neighbouring cells and their gathers share cache lines.  The class table is staged in LDS when it
//                      fits kClassLdsBudget and read from global memory otherwise - the same code apart from the pointer.  The one
//                      barrier stands before the march; inside it a lane whose ray has ended idles until a ballot says that the wave
//                      is done.  Every output element is written exactly once, by its own lane, without atomics: the result depends
//                      on neither the launch geometry nor on how the views are split over launches.
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "raycast_rules.h"

namespace vray {

struct BricksArgs {
    int nx, ny, nz;
    float min_weight;
    const float* tsdf;                     // [nx][ny][nz]
    const float* weight;                   // [nx][ny][nz]
    unsigned char* bricks;                 // [bx][by][bz]
};

__global__ void __launch_bounds__(kBricksWG) tsdf_bricks(BricksArgs a) {
    const int by = rc::brick_dim(a.ny), bz = rc::brick_dim(a.nz);
    const int A = (int)blockIdx.x / by, B = (int)blockIdx.x % by;
    const int lane = threadIdx.x & 63;
    for (int k0 = 0; k0 < a.nz - 1; k0 += kBricksWG) {     // the same trip count for every lane: ballots inside
        const int k = k0 + (int)threadIdx.x;               // the cell along k this lane owns: voxels k and k + 1
        const bool active = k < a.nz - 1;
        bool any_cell = false, all_free = true;
        unsigned prev = 0;
        for (int di = 0; di <= 8; ++di) {
            const int i = 8 * A + di;
            if (i > a.nx - 1) break;                       // uniform over the workgroup
            unsigned cur = 0;                              // bit dj: voxels (i, j, k) and (i, j, k + 1) are both valid
            for (int dj = 0; dj <= 8; ++dj) {
                const int j = 8 * B + dj;
                if (j > a.ny - 1) break;
                if (!active) continue;
                const long long p = ((long long)i * a.ny + j) * a.nz + k;      // k + 1 <= nz - 1
                const bool v0 = rc::voxel_valid(a.weight[p], a.min_weight), v1 = rc::voxel_valid(a.weight[p + 1], a.min_weight);
                if (v0 && v1) cur |= 1u << dj;
                all_free = all_free && v0 && v1 && rc::voxel_free(a.tsdf[p]) && rc::voxel_free(a.tsdf[p + 1]);
            }
            const unsigned both = prev & cur;              // rows of slab i - 1 and slab i; a row outside the volume left its bit 0
            any_cell = any_cell || (di > 0 && (both & (both >> 1)) != 0u);
            prev = cur;
        }
        const unsigned long long any_mask = __ballot(active && any_cell), bad_mask = __ballot(active && !all_free);
        if (active && (lane & 7) == 0) {                   // k0 and the wave's base are multiples of 8: this lane's k starts a brick
            const bool any = ((any_mask >> lane) & 0xffull) != 0ull, all = ((bad_mask >> lane) & 0xffull) == 0ull;
            a.bricks[((long long)A * by + B) * bz + (k >> rc::kBrickShift)] = rc::classify(any, all);
        }
    }
}

struct RaycastArgs {
    rc::Rules rules;
    rc::Volume vol;
    const unsigned char* bricks;           // null: the classes are not read
    int n_bricks;
    const float* views;                    // [n_views][12]
    int view0;                             // the first view of this launch
    float* depth;                          // [n_views][width][height]
    unsigned char* status;                 // [n_views][width][height]
    float* normal;                         // [n_views][width][height][3] or null
    unsigned char* color_out;              // [n_views][width][height][4] or null
};

__global__ void __launch_bounds__(kRaycastWG) tsdf_raycast(RaycastArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char staged[kClassLdsBudget];
    const unsigned char* table = a.bricks;
    if (a.bricks && a.n_bricks <= kClassLdsBudget) {       // uniform; the table's buffer is padded to 16 bytes (vmapstep_tsdf_bricks_bytes)
        const int n16 = (a.n_bricks + 15) / 16;
        for (int e = threadIdx.x; e < n16; e += kRaycastWG)
            reinterpret_cast<uint4*>(staged)[e] = reinterpret_cast<const uint4*>(a.bricks)[e];
        __syncthreads();
        table = staged;
    }
    const rc::Rules& r = a.rules;
    const int view = a.view0 + (int)blockIdx.y;
    const float* M = a.views + 12 * (long long)view;
    const int tiles_w = (r.width + kTile - 1) / kTile, tiles_h = (r.height + kTile - 1) / kTile;
    const int tile = (int)blockIdx.x * kTilesPerWG + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int w = tile / tiles_h * kTile + (lane >> 3), h = tile % tiles_h * kTile + (lane & 7);
    const bool own = tile < tiles_w * tiles_h && w < r.width && h < r.height;
    rc::Ray ray = {};
    rc::March m;
    rc::march_begin(m);
    int status = rc::MISS;
    float z = 0.0f;
    bool live = own && rc::make_ray(r, M, w, h, ray);
    while (__ballot(live) != 0ull) {                       // no barrier in here: waves of a workgroup finish on their own
        if (!live) continue;
        const int s = rc::march_step(r, a.vol, table, ray, m, z);
        if (s >= 0) {
            status = s;
            live = false;
        }
    }
    if (!own) return;
    const long long pix = ((long long)view * r.width + w) * r.height + h;
    const bool hit = status == rc::HIT;
    a.depth[pix] = hit ? z : 0.0f;
    a.status[pix] = (unsigned char)status;
    if (a.normal) {
        float n[3] = {0.0f, 0.0f, 0.0f};
        if (hit) rc::hit_normal(r, a.vol, ray, z, n);
        a.normal[3 * pix] = n[0];
        a.normal[3 * pix + 1] = n[1];
        a.normal[3 * pix + 2] = n[2];
    }
    if (a.color_out) {
        unsigned char c[4] = {0, 0, 0, 0};
        if (hit) rc::hit_color(r, a.vol, ray, z, c);
        reinterpret_cast<uchar4*>(a.color_out)[pix] = make_uchar4(c[0], c[1], c[2], c[3]);
    }
}

}  // namespace vray
