// raster_kernels.h - the mesh rasteriser on the device: depth and face images of an indexed triangle mesh from a set of poses, and the
// comparison of two depth stacks.  The rule (camera, snapping, coverage, depth, key, comparison) is raster_rules.h's; the contract is
// the raster section of include/vmapstep.h.
//
// One z-buffer pass: every covered (view, pixel) takes atomicMin of the 64-bit key (depth bits, face) on a [views][width][height] key
// image that starts as all ones.  A minimum does not depend on the order of arrival, so the images are a function of the input alone.
//
//   raster_setup       one lane per (view, face), one view per grid row: gather the corners through the index buffer (a face with an
//                      index out of range is dropped whole), transform, reject, snap (rr::setup_face), box the pixel centres.  A
//                      dropped face adds to dropped[view] (one atomic per wave).  A face whose box holds at most 4 x 4 centres is
//                      drawn here by its own lane: at most 16 coverage tests.  A larger face is only counted: 1 large face and the
//                      8 x 8 tiles its box touches, summed per block.
//   raster_scan        one workgroup: exclusive scans of both lists of block totals; the grand totals -> counts {large faces, pairs}
//   raster_emit        the same setup again; block scan + block offset -> the place of every large face and its first pair.  ONE
//                      record per large face whatever its area (the snapped corners, their depths, view, face, the tile rectangle),
//                      and nothing at or past large_cap.
//   raster_tiles       one wave per (view, face, tile) pair, one lane per pixel centre of the tile: the pair's face is found by a
//                      binary search of the first-pair list (rr::kTile x rr::kTile = one wave), at most ceil(log2(large faces)) steps.
//                      A pair index past the face's tile count (possible only with counts that are not the count call's) draws nothing.
//   raster_resolve     per pixel: key -> depth, face; label = face_labels[face]; face_seen[face] = 1 (byte stores of 1 only)
//   depth_compare      two depth stacks -> per view {n_both, n_a_only, n_b_only, sum_q}: integer sums, combined in the wave (shuffles)
//                      and the workgroup (LDS) before one set of global atomics per workgroup
// The per-lane bound: no loop's trip count depends on a face's screen area - 16 pixels in raster_setup, 1 pixel per pair in
// raster_tiles (and ceil(pairs / (4 x grid)) pairs per wave, 1 up to 4 M pairs), 1 record in raster_emit.
// Integer atomics only; nothing waits for another lane.
#pragma once
#include <hip/hip_runtime.h>

#include "component_rules.h"
#include "launch_geometry.h"
#include "raster_rules.h"
#include "scan_ops.h"

namespace vr {

struct LargeRec {                          // kLargeRecInts int32
    int X[3], Y[3];
    float z[3];
    int view, face;
    int tw0, th0, ntw, nth;                // the rectangle of tiles the face's box touches
    int pad;
};
static_assert(sizeof(LargeRec) == kLargeRecInts * sizeof(int), "one record = kLargeRecInts int32");

struct DrawArgs {
    rr::Camera cam;
    const float* vertices;                 // [n_vertices][3]
    long long n_vertices;
    const int* faces;                      // [n_faces][3]
    long long n_faces;
    const float* t_wc;                     // [slots][4][4]
    const int* slots;                      // [n_views] or null: view k reads slot k
    int n_views;
    int nfb;                               // blocks of kRasterWG faces per view
    unsigned long long* keys;              // [n_views][width][height]
    int* dropped;                          // [n_views]
    long long* blk;                        // workspace: [n_views * nfb][2] large faces and pairs per block, then their exclusive prefixes
    long long* counts;                     // device int64[2]: large faces, pairs
    long long* first;                      // [large_cap] the first pair of every large face
    LargeRec* recs;                        // [large_cap]
    long long large_cap;
    long long n_large, n_pairs;            // raster_tiles: records and pairs to draw
};

enum { kNone = 0, kDropped, kEmpty, kSmall, kLarge };

// the face of this lane in the view of this grid row: its class, the oriented face and its box
__device__ __forceinline__ int lane_face(const DrawArgs& a, long long face, int view, rr::Face& f, rr::Box& box) {
    if (face >= a.n_faces) return kNone;
    const int v0 = a.faces[3 * face], v1 = a.faces[3 * face + 1], v2 = a.faces[3 * face + 2];
    if (!kr::face_valid(v0, v1, v2, a.n_vertices)) return kDropped;
    const long long slot = a.slots ? a.slots[view] : view;
    const float* T = a.t_wc + 16 * slot;
    if (!rr::setup_face(a.cam, T, a.vertices + 3ll * v0, a.vertices + 3ll * v1, a.vertices + 3ll * v2, f)) return kDropped;
    box = rr::pixel_box(a.cam, f);
    if (rr::box_empty(box)) return kEmpty;
    return rr::box_small(box) ? kSmall : kLarge;
}

__device__ __forceinline__ void draw_pixel(const rr::Camera& cam, const rr::Face& f, int face, unsigned long long* image, int w, int h) {
    long long E[3];
    if (!rr::covers(f, w, h, E)) return;
    const float z = rr::depth_at(f, E);
    if (!rr::depth_written(cam, z)) return;
    atomicMin(image + ((long long)w * cam.height + h), rr::make_key(z, face));
}

__device__ __forceinline__ long long tiles_of(const rr::Box& b) {
    return (long long)((b.w1 / rr::kTile) - (b.w0 / rr::kTile) + 1) * ((b.h1 / rr::kTile) - (b.h0 / rr::kTile) + 1);
}

__global__ void __launch_bounds__(kRasterWG) raster_setup(DrawArgs a) {
    __shared__ long long wsum_l[kRasterWG / 64], wsum_p[kRasterWG / 64];
    const long long face = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    const int view = blockIdx.y;
    rr::Face f;
    rr::Box box;
    const int cls = lane_face(a, face, view, f, box);
    const unsigned long long gone = __ballot(cls == kDropped);
    if ((threadIdx.x & 63) == 0 && gone != 0ull) atomicAdd(a.dropped + view, __popcll(gone));
    if (cls == kSmall) {
        unsigned long long* image = a.keys + (long long)view * a.cam.width * a.cam.height;
        for (int w = box.w0; w <= box.w1; ++w)             // at most rr::kSmallSide x rr::kSmallSide centres
            for (int h = box.h0; h <= box.h1; ++h) draw_pixel(a.cam, f, (int)face, image, w, h);
    }
    const long long large = cls == kLarge ? 1 : 0, pairs = cls == kLarge ? tiles_of(box) : 0;
    long long total_l, total_p;
    (void)vscan::wg_exclusive_scan<kRasterWG>(large, wsum_l, total_l);
    (void)vscan::wg_exclusive_scan<kRasterWG>(pairs, wsum_p, total_p);
    if (threadIdx.x == 0) {
        const long long b = (long long)view * a.nfb + blockIdx.x;
        a.blk[2 * b] = total_l;
        a.blk[2 * b + 1] = total_p;
    }
}

__global__ void __launch_bounds__(kRasterScanWG) raster_scan(DrawArgs a) {
    __shared__ long long wsum_l[kRasterScanWG / 64], wsum_p[kRasterScanWG / 64];
    const long long nblk = (long long)a.n_views * a.nfb;
    // Both lists in one walk, kScanPer consecutive blocks per lane: 20 views of 0.9 M faces are 70 k blocks, this one workgroup is on
    // the call's critical path, and a round costs its chain of load -> barrier -> store whatever it carries (one block per lane and
    // round: 0.20 ms, HISTORY.md).
    long long nl = 0, np = 0;
    for (long long base = 0; base < nblk; base += (long long)kRasterScanWG * kScanPer) {
        const long long b0 = base + (long long)threadIdx.x * kScanPer;
        long long xl[kScanPer], xp[kScanPer], sl = 0, sp = 0;
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            xl[j] = b0 + j < nblk ? a.blk[2 * (b0 + j)] : 0;
            xp[j] = b0 + j < nblk ? a.blk[2 * (b0 + j) + 1] : 0;
            sl += xl[j];
            sp += xp[j];
        }
        long long total_l, total_p;
        long long rl = nl + vscan::wg_exclusive_scan<kRasterScanWG>(sl, wsum_l, total_l);
        long long rp = np + vscan::wg_exclusive_scan<kRasterScanWG>(sp, wsum_p, total_p);
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            if (b0 + j < nblk) { a.blk[2 * (b0 + j)] = rl; a.blk[2 * (b0 + j) + 1] = rp; }
            rl += xl[j];
            rp += xp[j];
        }
        nl += total_l;
        np += total_p;
        __syncthreads();                                   // both wsum arrays are rewritten by the next round
    }
    if (threadIdx.x == 0) { a.counts[0] = nl; a.counts[1] = np; }
}

__global__ void __launch_bounds__(kRasterWG) raster_emit(DrawArgs a) {
    __shared__ long long wsum_l[kRasterWG / 64], wsum_p[kRasterWG / 64];
    const long long face = (long long)blockIdx.x * kRasterWG + threadIdx.x;
    const int view = blockIdx.y;
    rr::Face f;
    rr::Box box;
    const int cls = lane_face(a, face, view, f, box);
    const long long large = cls == kLarge ? 1 : 0, pairs = cls == kLarge ? tiles_of(box) : 0;
    long long total_l, total_p;
    const long long b = (long long)view * a.nfb + blockIdx.x;
    const long long at = a.blk[2 * b] + vscan::wg_exclusive_scan<kRasterWG>(large, wsum_l, total_l);
    const long long first = a.blk[2 * b + 1] + vscan::wg_exclusive_scan<kRasterWG>(pairs, wsum_p, total_p);
    if (cls == kLarge && at < a.large_cap) {
        LargeRec r;
#pragma unroll
        for (int c = 0; c < 3; ++c) { r.X[c] = f.X[c]; r.Y[c] = f.Y[c]; r.z[c] = f.z[c]; }
        r.view = view; r.face = (int)face;
        r.tw0 = box.w0 / rr::kTile; r.th0 = box.h0 / rr::kTile;
        r.ntw = box.w1 / rr::kTile - r.tw0 + 1; r.nth = box.h1 / rr::kTile - r.th0 + 1;
        r.pad = 0;
        a.recs[at] = r;
        a.first[at] = first;
    }
}

__global__ void __launch_bounds__(kRasterWG) raster_tiles(DrawArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * kTilesPerWG;
    for (long long pair = (long long)blockIdx.x * kTilesPerWG + wave; pair < a.n_pairs; pair += stride) {
        const long long r = vscan::segment_of(a.first, (int)a.n_large, pair);       // wave-uniform: first[0] == 0 <= pair
        const LargeRec rec = a.recs[r];
        const long long t = pair - a.first[r];
        // a record the emit did not write is all zero (the draw call clears the buffer): no tile, nothing drawn
        if (t < 0 || t >= (long long)rec.ntw * rec.nth || rec.view < 0 || rec.view >= a.n_views) continue;
        const int tw = rec.tw0 + (int)(t % rec.ntw), th = rec.th0 + (int)(t / rec.ntw);
        const int w = tw * rr::kTile + (lane >> 3), h = th * rr::kTile + (lane & 7);       // h is the fast index of the image
        if ((unsigned)w >= (unsigned)a.cam.width || (unsigned)h >= (unsigned)a.cam.height) continue;
        rr::Face f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { f.X[c] = rec.X[c]; f.Y[c] = rec.Y[c]; f.z[c] = rec.z[c]; }
        f.A = rr::edge_fn(f.X[0], f.Y[0], f.X[1], f.Y[1], f.X[2], f.Y[2]);         // the record is oriented: A > 0
        draw_pixel(a.cam, f, rec.face, a.keys + (long long)rec.view * a.cam.width * a.cam.height, w, h);
    }
}

struct ResolveArgs {
    const unsigned long long* keys;        // [n_pixels]
    long long n_pixels;
    float* depth;                          // [n_pixels]
    int* face;                             // [n_pixels]
    const int* face_labels;                // [n_faces] or null
    long long n_faces;
    int* label;                            // [n_pixels] or null
    unsigned char* face_seen;              // [n_faces] or null
};

__global__ void __launch_bounds__(kResolveWG) raster_resolve(ResolveArgs a) {
    const long long i = (long long)blockIdx.x * kResolveWG + threadIdx.x;
    if (i >= a.n_pixels) return;
    const unsigned long long key = a.keys[i];
    int face = rr::key_face(key);
    if (!(face >= 0 && face < a.n_faces)) face = -1;       // a key nobody of this family wrote: empty
    a.depth[i] = face < 0 ? 0.0f : rr::key_depth(key);
    a.face[i] = face;
    if (a.label) a.label[i] = face < 0 || !a.face_labels ? -1 : a.face_labels[face];
    if (a.face_seen && face >= 0) a.face_seen[face] = 1;
}

struct CompareArgs {
    const float* a;                        // [n_views][pixels]
    const float* b;
    long long pixels;
    unsigned long long* out;               // [n_views][kCompareInts] (int64 to the caller)
};

__global__ void __launch_bounds__(kCompareWG) depth_compare(CompareArgs a) {
    __shared__ unsigned long long part[kCompareWG / 64][kCompareInts];
    const long long base = (long long)blockIdx.y * a.pixels;
    unsigned long long s[kCompareInts] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kComparePer; ++j) {
        const long long i = (long long)blockIdx.x * kCompareBlock + j * kCompareWG + threadIdx.x;
        if (i >= a.pixels) continue;
        const float x = a.a[base + i], y = a.b[base + i];
        const int c = rr::compare_class(x, y);
        if (c == rr::kBoth) { s[0] += 1; s[3] += (unsigned long long)rr::compare_q(x, y); }
        else if (c == rr::kAOnly) s[1] += 1;
        else if (c == rr::kBOnly) s[2] += 1;
    }
#pragma unroll
    for (int k = 0; k < kCompareInts; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kCompareInts; ++k) part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kCompareInts) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kCompareWG / 64; ++w) t += part[w][threadIdx.x];
        if (t != 0) atomicAdd(a.out + (long long)blockIdx.y * kCompareInts + threadIdx.x, t);
    }
}

}  // namespace vr
