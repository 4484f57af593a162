// icp_kernels.h - the depth tracker on the device: frame-to-model projective ICP of a depth image against a model depth image.  The
// rules (pyramid, maps, correspondence, quantised sums, solve and update) are icp_rules.h's; the contract is the icp section of
// include/vmapstep.h.
//
//   icp_pyramid   one launch per level, one pixel of the output level per lane, tiles of kTileW x kTileH with h the fast axis.  The
//                 tile's depths with a one-pixel halo go to LDS first - level 0: the input cleaned; level l + 1: icp::down of the 2 x 2
//                 block of level l, halo pixels computed again by the neighbouring tile rather than exchanged - then every lane takes
//                 its normal from the five LDS values and writes ONE 16-byte entry (n0, n1, n2, d).  That entry is all a
//                 correspondence reads of either side: the model's point is rebuilt from d and the pixel index.
//   icp_reduce    the hot path.  A grid sized to the machine (at most kReduceGrid workgroups) strides over the source pixels; a lane
//                 rebuilds the source point in registers from its entry, transforms, projects, gathers ONE model entry and adds the
//                 pair's 29 integers to registers.  After the loop: 29 x 6 64-bit xor-shuffles in the wave, the four waves' rows
//                 through LDS, one set of 29 64-bit integer atomics per workgroup (zeros skipped).  Integer sums only: the result
//                 does not depend on the schedule.  A finished level's launches test the flag at entry - every wave of the grid
//                 reads the same word - and return.
//   icp_solve     one wave, lane 0: icp::solve on the 29 sums, the new pose, the iteration's rows of the three logs, the finished
//                 flag, and the sums back to zero for the next icp_reduce.
// A track call is a fixed chain of these launches on one stream; nothing waits for the host.
#pragma once
#include <hip/hip_runtime.h>

#include "icp_rules.h"
#include "launch_geometry.h"

namespace vi {

struct PyramidArgs {
    icp::Rules rules;
    icp::Camera cam;                       // the output level's
    const float* src;                      // level 0: the input depth; else the d component of the level below's first entry
    int src_stride;                        // floats between two pixels of src: 1 or 4
    int src_w, src_h;
    int first;                             // the output is level 0
    float4* out;                           // [cam.width][cam.height]
};

__global__ void __launch_bounds__(kPyramidWG) icp_pyramid(PyramidArgs a) {
    __shared__ float tile[kTileW + 2][kTileH + 2];
    const int w0 = blockIdx.x * kTileW, h0 = blockIdx.y * kTileH;
    for (int i = threadIdx.x; i < (kTileW + 2) * (kTileH + 2); i += kPyramidWG) {
        const int tw = i / (kTileH + 2), th = i - tw * (kTileH + 2);
        const int w = w0 + tw - 1, h = h0 + th - 1;
        float d = 0.0f;
        if (w >= 0 && w < a.cam.width && h >= 0 && h < a.cam.height) {
            if (a.first) {
                d = icp::clean(a.rules, a.src[((long long)w * a.src_h + h) * a.src_stride]);
            } else {
                const int wa = 2 * w, ha = 2 * h;      // < src_w, src_h: w < ceil(src_w / 2)
                const int wb = wa + 1 < a.src_w ? wa + 1 : a.src_w - 1, hb = ha + 1 < a.src_h ? ha + 1 : a.src_h - 1;
                const float d0 = a.src[((long long)wa * a.src_h + ha) * a.src_stride], d1 = a.src[((long long)wb * a.src_h + ha) * a.src_stride];
                const float d2 = a.src[((long long)wa * a.src_h + hb) * a.src_stride], d3 = a.src[((long long)wb * a.src_h + hb) * a.src_stride];
                d = icp::down(a.rules, d0, d1, d2, d3);
            }
        }
        tile[tw][th] = d;
    }
    __syncthreads();
    const int tw = threadIdx.x / kTileH, th = threadIdx.x - tw * kTileH;
    const int w = w0 + tw, h = h0 + th;
    if (w >= a.cam.width || h >= a.cam.height) return;
    float n[3];
    const float d = tile[tw + 1][th + 1];
    icp::normal(a.rules, a.cam, w, h, d, tile[tw][th + 1], tile[tw + 2][th + 1], tile[tw + 1][th], tile[tw + 1][th + 2], n);
    a.out[(long long)w * a.cam.height + h] = make_float4(n[0], n[1], n[2], d);
}

struct ReduceArgs {
    icp::Rules rules;
    icp::Camera cam;                       // the level's; source and model share it
    const float4* src;
    const float4* model;
    const double* pose;                    // [12] source camera -> model camera
    const int* done;                       // the level's finished flag, or null
    unsigned long long* sums;              // [kSums] (int64 to everyone else)
    int n_pix;
};

__global__ void __launch_bounds__(kReduceWG) icp_reduce(ReduceArgs a) {
    __shared__ unsigned long long part[kReduceWG / 64][kSums];
    if (a.done && *a.done) return;
    float T[12];
    icp::pose_rows(a.pose, T);
    long long s[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0;
    const int H = a.cam.height;
    const int stride = (int)gridDim.x * kReduceWG;       // n_pix <= 2^20 and stride <= 2^18: no overflow
    for (int i = (int)blockIdx.x * kReduceWG + (int)threadIdx.x; i < a.n_pix; i += stride) {
        const float4 e = a.src[i];
        const int w = i / H, h = i - w * H;
        const float sv[4] = {e.x, e.y, e.z, e.w};
        float pp[3], np[3];
        int wm = 0, hm = 0;
        if (icp::project(a.rules, a.cam, T, w, h, sv, pp, np, wm, hm) != icp::INLIER) continue;
        const float4 m = a.model[(long long)wm * H + hm];                // wm, hm inside the level: icp::project checked
        const float mv[4] = {m.x, m.y, m.z, m.w};
        icp::Pair p;
        if (icp::residual(a.rules, a.cam, pp, np, wm, hm, mv, p) != icp::INLIER) continue;
        icp::accumulate(p, s);
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) part[wave][k] = (unsigned long long)s[k];
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        unsigned long long t = 0;
#pragma unroll
        for (int v = 0; v < kReduceWG / 64; ++v) t += part[v][threadIdx.x];
        if (t != 0) atomicAdd(a.sums + threadIdx.x, t);
    }
}

struct SolveArgs {
    icp::Solve p;
    unsigned long long* sums;              // [kSums]; zero again on return
    double* pose;                          // [12]
    int* done;
    double* log;                           // this iteration's row [icp::kLogCols], or null
    long long* sums_log;                   // [kSums], or null
    double* pose_log;                      // [12], or null
    int last_of_level;                     // the flag is lowered for the next level
};

__global__ void __launch_bounds__(kSolveWG) icp_solve(SolveArgs a) {
    if (threadIdx.x != 0) return;
    const bool skipped = *a.done != 0;
    long long s[kSums];
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = a.pose[k];
    icp::Step st;
    st.status = icp::SKIPPED;
    st.finished = 0;
    st.x2 = 0.0;
    for (int k = 0; k < kSums; ++k) s[k] = 0;
    if (!skipped) {
        for (int k = 0; k < kSums; ++k) {
            s[k] = (long long)a.sums[k];
            a.sums[k] = 0;
        }
        icp::solve(a.p, s, T, st);
        for (int k = 0; k < 12; ++k) a.pose[k] = T[k];
    }
    if (a.log) {
        a.log[0] = (double)s[0];
        a.log[1] = (double)s[28] * (1.0 / icp::kQuant);
        a.log[2] = (double)st.status;
        a.log[3] = st.x2;
    }
    if (a.sums_log)
        for (int k = 0; k < kSums; ++k) a.sums_log[k] = s[k];
    if (a.pose_log)
        for (int k = 0; k < 12; ++k) a.pose_log[k] = T[k];
    if (a.last_of_level) *a.done = 0;
    else if (st.finished) *a.done = 1;
}

}  // namespace vi
