// cull_kernels.h - visibility culling on the device: which points of a cloud (the vertices of a mesh, or samples of its surface) any
// of a set of keyframes saw, and the compaction of a mesh by such a mask.  The rule is cull_rules.h's; the contract is the cull
// section of include/vmapstep.h.
//
//   cull_mark          a lane owns kPointsPer points in registers (kCullWG apart, so a wave's 64 points are consecutive: marching-cubes
//                      vertex order is spatially coherent and a wave's depth gathers share cache lines).  The `seen` byte is read
//                      first: a point that is seen already is never tested.  The grid is (point tiles, frame chunks), tiles the fast
//                      dimension: the workgroups in flight together work on the same kFrameChunk frames, whose depth images (3.26 MB
//                      each at 1200 x 680) then compete for an XCD's 4 MiB L2 a few at a time and not all K at once - reasoning, not
//                      measurement; tests/tools/cull_bench.py is the measurement.  A workgroup stages the chunk's poses and image
//                      offsets in LDS and loops over the frames; a wave leaves the loop once a ballot says all its lanes are seen.
//                      The only write is a byte store of the value 1, the same from every writer (workgroups of different chunks
//                      own the same points), so the result is a set: independent of order and of what a racing read of `seen` saw.
//   cull_clear         the referenced byte of every vertex = 0
//   cull_face_count    per face: kept iff at least min_seen corners are seen (and every index names a vertex); a kept face marks
//                      its three vertices referenced (byte stores of 1); the block's kept faces
//   cull_vertex_count  the block's referenced vertices
//   cull_scan          one workgroup: exclusive scans of both lists of block totals; the two grand totals -> counts
//   cull_vertex_emit   block scan + block offset -> the new index of every referenced vertex; kept_vertices[new] = old
//   cull_face_emit     block scan + block offset -> the place of every kept face; its corners re-indexed
// Everything the compaction combines is an integer sum, and places follow face order and ascending old vertex index: the output is
// bit-identical from call to call.
#pragma once
#include <hip/hip_runtime.h>

#include "cull_rules.h"
#include "launch_geometry.h"
#include "scan_ops.h"

namespace vc {

struct MarkArgs {
    cr::Rules rules;
    const float* points;                   // [n_points][3]
    long long n_points;
    const float* depth;                    // [slots][width][height]; null in frustum-only mode
    const float* t_wc;                     // [slots][4][4]
    const int* slots;                      // [n_frames] or null: frame k reads slot k
    int n_frames;
    unsigned char* seen;                   // [n_points]
};

__global__ void __launch_bounds__(kCullWG) cull_mark(MarkArgs a) {
    __shared__ float pose[kFrameChunk][12];
    __shared__ long long image[kFrameChunk];
    const long long tile0 = (long long)blockIdx.x * kCullTile;
    float px[kPointsPer], py[kPointsPer], pz[kPointsPer];
    bool open[kPointsPer];                                 // the point exists and nobody has seen it yet
#pragma unroll
    for (int j = 0; j < kPointsPer; ++j) {
        const long long i = tile0 + j * kCullWG + threadIdx.x;
        open[j] = i < a.n_points && a.seen[i] == 0;
        px[j] = py[j] = pz[j] = 0.0f;
        if (open[j]) { px[j] = a.points[3 * i]; py[j] = a.points[3 * i + 1]; pz[j] = a.points[3 * i + 2]; }
    }
    const long long pixels = (long long)a.rules.width * a.rules.height;
    const int n_chunks = (a.n_frames + kFrameChunk - 1) / kFrameChunk;
    for (int chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {      // the same trip count for every lane: barriers inside
        const int k0 = chunk * kFrameChunk;
        const int nk = a.n_frames - k0 < kFrameChunk ? a.n_frames - k0 : kFrameChunk;
        __syncthreads();                                   // the previous chunk's poses are no longer read
        for (int e = threadIdx.x; e < nk * 12; e += kCullWG) {
            const int f = e / 12, c = e - 12 * f;
            const long long slot = a.slots ? a.slots[k0 + f] : k0 + f;
            pose[f][c] = a.t_wc[16 * slot + c];
            if (c == 0) image[f] = slot * pixels;           // 64-bit: slots * width * height passes 2^31 at realistic sizes
        }
        __syncthreads();
        for (int f = 0; f < nk; ++f) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < kPointsPer; ++j) any |= open[j];
            if (__ballot(any) == 0ull) break;              // wave-uniform: every lane of this wave is seen (or owns no point)
#pragma unroll
            for (int j = 0; j < kPointsPer; ++j) {
                if (!open[j]) continue;
                int w = 0, h = 0;
                float z = 0.0f;
                if (!cr::project(a.rules, pose[f], px[j], py[j], pz[j], w, h, z)) continue;
                if (a.rules.use_depth && !cr::not_occluded(z, a.depth[image[f] + cr::pixel_offset(a.rules, w, h)], a.rules.eps)) continue;
                open[j] = false;
                a.seen[tile0 + j * kCullWG + threadIdx.x] = 1;
            }
        }
    }
}

struct CompactArgs {
    const int* faces;                      // [n_faces][3]
    long long n_faces;
    const unsigned char* seen;             // [n_vertices]
    long long n_vertices;
    int min_seen;
    int nfb, nvb;
    unsigned char* used;                   // workspace: [n_vertices] referenced by a kept face
    int* newidx;                           // workspace: [n_vertices] the new index of a referenced vertex
    long long* fblk;                       // workspace: [nfb] kept faces per block, then their exclusive prefix
    long long* vblk;                       // workspace: [nvb] referenced vertices per block, then their exclusive prefix
    long long* counts;                     // device int64[2]: kept faces, kept vertices
    int* kept_vertices;                    // [vertex_cap]
    int* faces_out;                        // [face_cap][3]
    long long vertex_cap, face_cap;
};

// the corners of face `face` and whether it is kept; a face with an index outside [0, n_vertices) is dropped
__device__ __forceinline__ bool load_face(const CompactArgs& a, long long face, int (&v)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = a.faces[3 * face + c];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) ok = ok && v[c] >= 0 && v[c] < a.n_vertices;
    if (!ok) return false;
    return cr::face_kept(a.seen[v[0]], a.seen[v[1]], a.seen[v[2]], a.min_seen);
}

__global__ void __launch_bounds__(kCullWG) cull_clear(CompactArgs a) {
    const long long v = (long long)blockIdx.x * kCullWG + threadIdx.x;
    if (v < a.n_vertices) a.used[v] = 0;
}

__global__ void __launch_bounds__(kCullWG) cull_face_count(CompactArgs a) {
    __shared__ int wsum[kCullWG / 64];
    const long long face = (long long)blockIdx.x * kCullWG + threadIdx.x;
    int v[3];
    const int kept = face < a.n_faces && load_face(a, face, v) ? 1 : 0;
    if (kept) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.used[v[c]] = 1;
    }
    int total;
    (void)vscan::wg_exclusive_scan<kCullWG>(kept, wsum, total);
    if (threadIdx.x == 0) a.fblk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kCullWG) cull_vertex_count(CompactArgs a) {
    __shared__ int wsum[kCullWG / 64];
    const long long v = (long long)blockIdx.x * kCullWG + threadIdx.x;
    const int used = v < a.n_vertices && a.used[v] ? 1 : 0;
    int total;
    (void)vscan::wg_exclusive_scan<kCullWG>(used, wsum, total);
    if (threadIdx.x == 0) a.vblk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kCullScanWG) cull_scan(CompactArgs a) {
    __shared__ long long wsum[kCullScanWG / 64];
    // wg_scan_totals ends every chunk with a barrier: wsum is free again when the second scan starts
    const long long nf = vscan::wg_scan_totals<kCullScanWG>(
        a.nfb, wsum, [&](long long b) { return a.fblk[b]; }, [&](long long b, long long ex) { a.fblk[b] = ex; });
    const long long nv = vscan::wg_scan_totals<kCullScanWG>(
        a.nvb, wsum, [&](long long b) { return a.vblk[b]; }, [&](long long b, long long ex) { a.vblk[b] = ex; });
    if (threadIdx.x == 0) { a.counts[0] = nf; a.counts[1] = nv; }
}

__global__ void __launch_bounds__(kCullWG) cull_vertex_emit(CompactArgs a) {
    __shared__ int wsum[kCullWG / 64];
    const long long v = (long long)blockIdx.x * kCullWG + threadIdx.x;
    const int used = v < a.n_vertices && a.used[v] ? 1 : 0;
    int total;
    const long long at = a.vblk[blockIdx.x] + vscan::wg_exclusive_scan<kCullWG>(used, wsum, total);
    if (used) {
        a.newidx[v] = (int)at;
        if (at < a.vertex_cap) a.kept_vertices[at] = (int)v;
    }
}

__global__ void __launch_bounds__(kCullWG) cull_face_emit(CompactArgs a) {
    __shared__ int wsum[kCullWG / 64];
    const long long face = (long long)blockIdx.x * kCullWG + threadIdx.x;
    int v[3] = {0, 0, 0};
    const int kept = face < a.n_faces && load_face(a, face, v) ? 1 : 0;
    int total;
    const long long at = a.fblk[blockIdx.x] + vscan::wg_exclusive_scan<kCullWG>(kept, wsum, total);
    if (kept && at < a.face_cap) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.faces_out[3 * at + c] = a.newidx[v[c]];
    }
}

}  // namespace vc
