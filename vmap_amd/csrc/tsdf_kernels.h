// tsdf_kernels.h - TSDF fusion on the device: posed depth frames (a FrameStore in place), optionally masked to one object, folded into a
// truncated signed distance volume and a colour volume.  The rule is tsdf_rules.h's; the contract is the tsdf section of
// include/vmapstep.h.
//
//   tsdf_integrate     a lane owns kVoxelsPer voxels (kTsdfWG apart, so a wave's 64 voxels are consecutive in the linear index, that is
//                      along k, the fast axis: their loads and stores of D, W and the colour are coalesced, and neighbouring voxels
//                      project onto neighbouring pixels, so a wave's depth gathers share cache lines).  D, W and the colour stay in
//                      registers over ALL frames of the call: the volume is read once and written once per call, whatever the number
//                      of frames - a wave whose 64 voxels nobody updated writes nothing, any other writes whole cache lines.  A workgroup stages the poses and image offsets of
//                      kTsdfChunk frames in LDS at a time.  Per frame and voxel slot a wave votes (ballot) after the projection and
//                      skips the gather when none of its lanes landed in the image.  No atomics, no hand-off between workgroups:
//                      the result depends on the frame order alone (tsdf_rules.h, properties 1 and 2).
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "tsdf_rules.h"

namespace vtsdf {

struct IntegrateArgs {
    tr::Rules rules;
    int nx, ny, nz, n;                     // n = nx * ny * nz (< 2^31 / 3, the mesh ABI's limit)
    float A[12];                           // voxel index -> world, rows [A | b]
    float* tsdf;                           // [n]
    float* weight;                         // [n]
    float* color;                          // [n][4] r, g, b, wc; null without colour
    const float* depth;                    // [slots][width][height]
    const unsigned char* rgbx;             // [slots][width][height][4]; read only with colour
    const int* inst;                       // [slots][width][height]; read only with rules.obj_id >= 0
    const float* t_wc;                     // [slots][4][4]
    const int* slots;                      // [n_frames] or null: frame k reads slot k
    int n_frames;
};

template <bool COLOR>
__global__ void __launch_bounds__(kTsdfWG) tsdf_integrate(IntegrateArgs a) {
    __shared__ float pose[kTsdfChunk][12];
    __shared__ long long image[kTsdfChunk];
    const int tile0 = blockIdx.x * kTsdfTile;              // < n + kTsdfTile: fits an int (n < 2^31 / 3)
    float px[kVoxelsPer], py[kVoxelsPer], pz[kVoxelsPer], D[kVoxelsPer], W[kVoxelsPer];
    float C[kVoxelsPer][4];
    bool own[kVoxelsPer], dirty[kVoxelsPer];
#pragma unroll
    for (int j = 0; j < kVoxelsPer; ++j) {
        const int p = tile0 + j * kTsdfWG + (int)threadIdx.x;
        own[j] = p < a.n;
        dirty[j] = false;
        px[j] = py[j] = pz[j] = D[j] = W[j] = 0.0f;
        C[j][0] = C[j][1] = C[j][2] = C[j][3] = 0.0f;
        if (own[j]) {
            const int k = p % a.nz, r = p / a.nz;
            tr::voxel_center(a.A, r / a.ny, r % a.ny, k, px[j], py[j], pz[j]);
            D[j] = a.tsdf[p];
            W[j] = a.weight[p];
            if (COLOR) {
                const float4 c = reinterpret_cast<const float4*>(a.color)[p];
                C[j][0] = c.x; C[j][1] = c.y; C[j][2] = c.z; C[j][3] = c.w;
            }
        }
    }
    const long long pixels = (long long)a.rules.cam.width * a.rules.cam.height;
    for (int k0 = 0; k0 < a.n_frames; k0 += kTsdfChunk) {  // the same trip count for every lane: barriers inside
        const int nk = a.n_frames - k0 < kTsdfChunk ? a.n_frames - k0 : kTsdfChunk;
        __syncthreads();                                   // the previous chunk's poses are no longer read
        for (int e = threadIdx.x; e < nk * 12; e += kTsdfWG) {
            const int f = e / 12, c = e - 12 * f;
            const long long slot = a.slots ? a.slots[k0 + f] : k0 + f;
            pose[f][c] = a.t_wc[16 * slot + c];
            if (c == 0) image[f] = slot * pixels;           // 64-bit: slots * width * height passes 2^31 at realistic sizes
        }
        __syncthreads();
        for (int f = 0; f < nk; ++f) {
#pragma unroll
            for (int j = 0; j < kVoxelsPer; ++j) {
                int w = 0, h = 0;
                float z = 0.0f;
                const bool hit = own[j] && cr::project(a.rules.cam, pose[f], px[j], py[j], pz[j], w, h, z);
                if (__ballot(hit) == 0ull) continue;       // wave-uniform: no lane of this wave landed in the image
                if (!hit) continue;
                const long long pix = cr::pixel_offset(a.rules.cam, w, h);
                float sdf = 0.0f;
                if (!tr::measure(a.rules, a.depth + image[f], a.inst ? a.inst + image[f] : nullptr, pix, z, sdf)) continue;
                tr::update(a.rules, sdf, D[j], W[j]);
                if (COLOR && tr::in_band(a.rules, sdf)) tr::update_color(a.rules, a.rgbx + 4 * (image[f] + pix), C[j]);
                dirty[j] = true;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kVoxelsPer; ++j) {
        // Wave-uniform: a wave stores its 64 voxels iff one of them was updated - whole cache lines or nothing.  Stores under a lane's
        // own flag leave partial lines and measured 15 to 25 % slower over 20 frames (HISTORY.md); an untouched voxel that is stored
        // gets the bits it was loaded with.
        if (__ballot(dirty[j]) == 0ull || !own[j]) continue;
        const int p = tile0 + j * kTsdfWG + (int)threadIdx.x;
        a.tsdf[p] = D[j];
        a.weight[p] = W[j];
        if (COLOR) reinterpret_cast<float4*>(a.color)[p] = make_float4(C[j][0], C[j][1], C[j][2], C[j][3]);
    }
}

}  // namespace vtsdf
