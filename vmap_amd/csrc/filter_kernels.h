// filter_kernels.h - the instance filter on the device: what ScanNet's box_filter (utils.py:112-208) does on the host per frame with
// one full-frame pass per instance (cv2.erode, Open3D unprojection, the inside test against the instance's box).  A decoded frame as
// the image files hold it (row-major [H, W]: depth u16 / f32, instance and class labels u16 / i32), the pose and the table of the
// boxes registered so far become the per-id table (statistics and status), the voxel keys that join the ids' clouds and the label
// image.  The rules are filter_rules.h's; the contract is the filter section of include/vmapstep.h.
//
// Everything blocks combine is an integer sum, minimum or maximum, and keys are written in pixel order, so the output is bit-identical
// from call to call:
//   filter_init     every copy of the global table = the identity of every statistic, overflow = 0
//   filter_stats    one workgroup per kTileW x kTileH tile.  The shifted ids of the tile and a halo of erode_radius are staged in LDS
//                   (-1: an id without a table row, -2: outside the image); a row pass marks the cells whose in-image row window is
//                   of one id, the column pass then asks that of every in-image row of the window, with the centre's id: "all equal
//                   over the window, clipped to the image".  Depth and class are read once, for the owned pixels; a valid pixel is
//                   unprojected and, where its id is known, tested against the id's box-table row.  The wave combines first (the
//                   first pending lane's id is broadcast, the lanes that match are balloted, the counts are popcounts of ballots),
//                   its leader adds to an LDS table keyed by id (kSlots slots, open addressing; no slot: the global table directly),
//                   and every used slot is flushed with integer atomics into copy (block % kReplicas) of the global table.  One
//                   byte of flags per pixel stays in the workspace for filter_emit
//   filter_decide   one workgroup: the copies merged, fr::decide, the status column, the present rows compacted in ascending id
//   filter_count    per block of kPixBlock pixels in pixel order: the pixels whose point joins a cloud (fr::emits), split into keys
//                   inside the grid and points outside it
//   filter_scan     one workgroup: exclusive scan of the blocks' key counts; the totals into the header
//   filter_emit     per block again: block scan + block offset -> each key's place
//   filter_write    the label image: fr::label_of by the status column; a MERGED id's pixels are tested against the box table again
//   voxel_points    one workgroup per segment of sorted keys: the voxel centres, and the segment's coordinate bounds from the
//                   integer extremes of its voxel coordinates (a centre is monotonic in its coordinate)
// 16-bit and 32-bit inputs are chosen by a wave-uniform branch on a flag of the argument block; the linear kernels load four
// consecutive pixels with one instruction where the pointers are 16-byte aligned.
#pragma once
#include <hip/hip_runtime.h>

#include "filter_loads.h"
#include "filter_rules.h"
#include "launch_geometry.h"
#include "scan_ops.h"

namespace vf {

// one run (or one flushed slot) into a row of statistics, in LDS or in global memory
__device__ __forceinline__ void accumulate(int* dst, int pixels, int c_lo, int c_hi, int valid, int inside, int eroded, int eroded_valid) {
    atomicAdd(dst + 0, pixels);
    atomicMin(dst + 1, c_lo);
    atomicMax(dst + 2, c_hi);
    if (valid) atomicAdd(dst + 3, valid);
    if (inside) atomicAdd(dst + 4, inside);
    if (eroded) atomicAdd(dst + 5, eroded);
    if (eroded_valid) atomicAdd(dst + 6, eroded_valid);
}

__global__ void __launch_bounds__(kFilterWG) filter_init(FilterArgs a) {
    const int i = blockIdx.x * kFilterWG + threadIdx.x;
    if (i < kReplicas * a.rules.max_ids * kTableInts) a.table[i] = stat_identity(i & (kTableInts - 1));
    if (i == 0) *a.overflow = 0;
}

__global__ void __launch_bounds__(kFilterWG) filter_stats(FilterArgs a) {
    __shared__ int ids[kHaloH][kHaloW + 1];
    __shared__ unsigned char rowrun[kHaloH][kTileW];
    __shared__ int key[kSlots];
    __shared__ int acc[kSlots][kTableInts];
    __shared__ int ovf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = a.rules.width, H = a.rules.height, r = a.rules.erode_radius;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int hw = kTileW + 2 * r, hh = kTileH + 2 * r;       // <= kHaloW, kHaloH: r <= kMaxRadius is checked before the launch
    if (tid < kSlots) {
        key[tid] = -1;
#pragma unroll
        for (int f = 0; f < kTableInts; ++f) acc[tid][f] = stat_identity(f);
    }
    if (tid == 0) ovf = 0;
    for (int i = tid; i < hw * hh; i += kFilterWG) {          // the tile and its halo: the shifted id, -1 or -2
        const int hy = i / hw, hx = i - hy * hw;
        const int y = y0 - r + hy, x = x0 - r + hx;
        int v = -2;
        if (x >= 0 && x < W && y >= 0 && y < H)
            v = fr::shifted_id(load_label(a.inst, (long long)y * W + x, a.label_i32), a.rules.id_shift, a.rules.max_ids);
        ids[hy][hx] = v;
    }
    __syncthreads();
    for (int i = tid; i < hh * kTileW; i += kFilterWG) {      // the row pass: the in-image cells of the row window carry the cell's id
        const int hy = i / kTileW, c = i - hy * kTileW;
        const int centre = ids[hy][c + r];
        bool ok = true;
        for (int dx = 0; dx <= 2 * r; ++dx) {
            const int v = ids[hy][c + dx];
            ok = ok && (v == centre || v == -2);
        }
        rowrun[hy][c] = ok ? 1 : 0;
    }
    __syncthreads();
    int* const table = a.table + (long long)((blockIdx.y * gridDim.x + blockIdx.x) % kReplicas) * a.rules.max_ids * kTableInts;
    constexpr int kRounds = kTileH / (kFilterWG / 64);
    for (int j = 0; j < kRounds; ++j) {                       // a wave owns 64 consecutive columns of one row
        const int ty = wave + j * (kFilterWG / 64), x = x0 + lane, y = y0 + ty;
        const bool active = x < W && y < H;
        const int id = ids[ty + r][lane + r];                 // -2 exactly where !active
        bool eroded = true;
        for (int dy = 0; dy <= 2 * r; ++dy) {                 // the column pass
            const int v = ids[ty + dy][lane + r];
            eroded = eroded && (v == -2 || (v == id && rowrun[ty + dy][lane] != 0));
        }
        int cls = 0;
        bool valid = false, inside = false;
        if (active) {
            const long long p = (long long)y * W + x;
            cls = load_label(a.sem, p, a.label_i32);
            const float d = ir::depth_of(load_depth(a.depth, p, a.depth_f32), a.rules.depth_scale, a.rules.max_depth);
            valid = fr::valid_depth(d);
            if (valid && id >= 0) {
                const float* row = a.box_table + (long long)id * fr::kBoxFloats;
                if (fr::box_known(row)) inside = fr::inside_box(row, fr::world_point(a.rules.cam, x, y, d));
            }
            a.flags[p] = (unsigned char)((valid ? fr::VALID : 0) | (inside ? fr::INSIDE : 0) | (eroded ? fr::ERODED : 0));
        }
        const bool counted = active && id >= 0;
        const unsigned long long lost = __ballot(active && id == -1);
        if (lost != 0 && lane == 0) atomicAdd(&ovf, __popcll(lost));
        unsigned long long todo = __ballot(counted);
        while (todo != 0) {                                   // wave-uniform: one round per id among the wave's pixels
            const int leader = __ffsll((long long)todo) - 1;
            const int lid = __shfl(id, leader, 64), lcls = __shfl(cls, leader, 64);
            const bool mine = counted && id == lid;
            const unsigned long long m = __ballot(mine);
            const int n_valid = __popcll(__ballot(mine && valid)), n_inside = __popcll(__ballot(mine && inside));
            const int n_eroded = __popcll(__ballot(mine && eroded)), n_ev = __popcll(__ballot(mine && eroded && valid));
            if (mine && cls != lcls) {                        // a second class on the id: rare, and an error for the caller
                atomicMin(table + (long long)id * kTableInts + 1, cls);
                atomicMax(table + (long long)id * kTableInts + 2, cls);
            }
            if (lane == leader) {
                int slot = -1;
                for (int k = 0; k < kProbes && slot < 0; ++k) {
                    const int s = (lid + k) & (kSlots - 1);
                    const int prev = atomicCAS(&key[s], -1, lid);
                    if (prev == -1 || prev == lid) slot = s;
                }
                int* dst = slot >= 0 ? acc[slot] : table + (long long)lid * kTableInts;
                accumulate(dst, __popcll(m), lcls, lcls, n_valid, n_inside, n_eroded, n_ev);
            }
            todo &= ~m;
        }
    }
    __syncthreads();
    if (tid < kSlots && key[tid] >= 0) {
        const int* s = acc[tid];
        accumulate(table + (long long)key[tid] * kTableInts, s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
    }
    if (tid == 0 && ovf != 0) atomicAdd(a.overflow, ovf);
}

__global__ void __launch_bounds__(kDecideWG) filter_decide(FilterArgs a) {
    __shared__ int wsum[kDecideWG / 64];
    const int max_ids = a.rules.max_ids;
    auto merged = [&](long long r) {
        fr::Stats s;
        s.pixels = s.valid = s.inside = s.eroded = s.eroded_valid = 0;
        s.c_min = kIntMax; s.c_max = kIntMin;
        for (int k = 0; k < kReplicas; ++k) {
            const int4* t = reinterpret_cast<const int4*>(a.table + ((long long)k * max_ids + r) * kTableInts);
            const int4 lo = t[0], hi = t[1];
            s.pixels += lo.x;
            s.c_min = min(s.c_min, lo.y); s.c_max = max(s.c_max, lo.z);
            s.valid += lo.w; s.inside += hi.x; s.eroded += hi.y; s.eroded_valid += hi.z;
        }
        return s;
    };
    fr::Stats s;                                              // of the row this lane holds in the current chunk
    const int n = vscan::wg_scan_totals<kDecideWG, int>(max_ids, wsum, [&](long long r) -> int {
        s = merged(r);
        return s.pixels > 0 ? 1 : 0;
    }, [&](long long r, int pos) {
        const int id = (int)r;
        const int st = fr::decide(a.rules, id, s, fr::box_known(a.box_table + r * fr::kBoxFloats));
        a.status[r] = st;
        if (s.pixels > 0) {
            int* o = a.rows_out + fr::kHeadInts + (long long)pos * fr::kRowInts;
            o[0] = id; o[1] = st; o[2] = s.c_min; o[3] = s.pixels;
            o[4] = s.valid; o[5] = s.inside; o[6] = s.eroded; o[7] = s.eroded_valid;
        }
    });
    if (threadIdx.x == 0) {
        a.rows_out[0] = n;
        a.rows_out[1] = *a.overflow;
        a.rows_out[2] = 0;
        a.rows_out[3] = 0;
    }
}

// the keys of this lane's pixels (bit c of the result: pixel c emits keys[c]); out: its points outside the grid
__device__ __forceinline__ int emit_lane(const FilterArgs& a, long long pix0, unsigned long long (&keys)[kPixPer], int& out) {
    int raw[kPixPer];
    float depth[kPixPer];
    out = 0;
    if (pix0 >= a.n_pix) return 0;
    load_labels4(a, a.inst, pix0, raw);
    load_depths4(a, pix0, depth);
    const int W = a.rules.width;
    int mask = 0;
#pragma unroll
    for (int c = 0; c < kPixPer; ++c) {
        const long long p = pix0 + c;
        if (p >= a.n_pix) break;
        const int id = fr::shifted_id(raw[c], a.rules.id_shift, a.rules.max_ids);
        if (id < 0 || !fr::emits(a.status[id], a.flags[p])) continue;
        const int v = (int)(p / W), u = (int)(p - (long long)v * W);
        const float d = ir::depth_of(depth[c], a.rules.depth_scale, a.rules.max_depth);
        if (fr::voxel_key(id, fr::world_point(a.rules.cam, u, v, d), a.rules.voxel, &keys[c])) mask |= 1 << c;
        else ++out;
    }
    return mask;
}

__global__ void __launch_bounds__(kFilterWG) filter_count(FilterArgs a) {
    __shared__ int wsum[kFilterWG / 64], wout[kFilterWG / 64];
    unsigned long long keys[kPixPer];
    int out;
    const int mask = emit_lane(a, ((long long)blockIdx.x * kFilterWG + threadIdx.x) * kPixPer, keys, out);
    int total, total_out;
    (void)vscan::wg_exclusive_scan<kFilterWG>(__builtin_popcount(mask), wsum, total);
    (void)vscan::wg_exclusive_scan<kFilterWG>(out, wout, total_out);
    if (threadIdx.x == 0) {
        a.blk[2 * blockIdx.x] = total;
        a.blk[2 * blockIdx.x + 1] = total_out;
    }
}

__global__ void __launch_bounds__(kDecideWG) filter_scan(FilterArgs a) {
    __shared__ int wsum[kDecideWG / 64];
    const int n_keys = vscan::wg_scan_totals<kDecideWG, int>(
        a.n_blk, wsum, [&](long long b) { return a.blk[2 * b]; }, [&](long long b, int ex) { a.blk[2 * b] = ex; });
    const int n_out = vscan::wg_scan_totals<kDecideWG, int>(
        a.n_blk, wsum, [&](long long b) { return a.blk[2 * b + 1]; }, [&](long long, int) {});
    if (threadIdx.x == 0) {
        a.rows_out[2] = n_keys;
        a.rows_out[3] = n_out;
    }
}

__global__ void __launch_bounds__(kFilterWG) filter_emit(FilterArgs a) {
    __shared__ int wsum[kFilterWG / 64];
    unsigned long long keys[kPixPer];
    int out;
    const int mask = emit_lane(a, ((long long)blockIdx.x * kFilterWG + threadIdx.x) * kPixPer, keys, out);
    int total;
    long long at = a.blk[2 * blockIdx.x] + vscan::wg_exclusive_scan<kFilterWG>(__builtin_popcount(mask), wsum, total);
#pragma unroll
    for (int c = 0; c < kPixPer; ++c)
        if (mask >> c & 1) {
            if (at < a.n_pix) a.keys_out[at] = keys[c];       // never false: at most one key per pixel
            ++at;
        }
}

__global__ void __launch_bounds__(kFilterWG) filter_write(FilterArgs a) {
    const long long pix0 = ((long long)blockIdx.x * kFilterWG + threadIdx.x) * kPixPer;
    if (pix0 >= a.n_pix) return;
    int raw[kPixPer], lab[kPixPer];
    float depth[kPixPer];
    load_labels4(a, a.inst, pix0, raw);
    load_depths4(a, pix0, depth);
    const int W = a.rules.width;
#pragma unroll
    for (int c = 0; c < kPixPer; ++c) {
        const long long p = pix0 + c;
        lab[c] = 0;
        if (p >= a.n_pix) break;
        const int id = fr::shifted_id(raw[c], a.rules.id_shift, a.rules.max_ids);
        if (id < 0) continue;
        const int st = a.status[id];
        bool valid = false, inside = false;
        if (st == fr::MERGED) {                               // against the box the id had when the frame arrived
            const float d = ir::depth_of(depth[c], a.rules.depth_scale, a.rules.max_depth);
            valid = fr::valid_depth(d);
            if (valid) {
                const int v = (int)(p / W), u = (int)(p - (long long)v * W);
                inside = fr::inside_box(a.box_table + (long long)id * fr::kBoxFloats, fr::world_point(a.rules.cam, u, v, d));
            }
        }
        lab[c] = fr::label_of(id, st, valid, inside);
    }
    if (a.vec_ok && pix0 + kPixPer <= a.n_pix) {
        *reinterpret_cast<int4*>(a.labels_out + pix0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
    } else {
#pragma unroll
        for (int c = 0; c < kPixPer; ++c)
            if (pix0 + c < a.n_pix) a.labels_out[pix0 + c] = lab[c];
    }
}

// ---- keys -> voxel centres --------------------------------------------------------------------------------------------------------

struct VoxelArgs {
    const unsigned long long* keys;        // [n_keys], sorted
    long long n_keys;
    const long long* offsets;              // [n_seg + 1] into keys
    int n_seg;
    float voxel;
    float* points;                         // [n_keys][3]
    float* bounds;                         // [n_seg][6]: the minimum, then the maximum of the segment's centres
};

__global__ void __launch_bounds__(kFilterWG) voxel_points(VoxelArgs a) {
    __shared__ int ext[6];
    const int s = blockIdx.x;
    if (threadIdx.x < 6) ext[threadIdx.x] = threadIdx.x < 3 ? kIntMax : kIntMin;
    __syncthreads();
    long long begin = a.offsets[s], end = a.offsets[s + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > a.n_keys ? a.n_keys : end;
    int lo[3] = {kIntMax, kIntMax, kIntMax}, hi[3] = {kIntMin, kIntMin, kIntMin};
    for (long long i = begin + threadIdx.x; i < end; i += kFilterWG) {
        const unsigned long long key = a.keys[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int q = fr::key_coord(key, k);
            a.points[3 * i + k] = fr::voxel_centre(q, a.voxel);
            lo[k] = min(lo[k], q);
            hi[k] = max(hi[k], q);
        }
    }
    if (begin + threadIdx.x < end) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(&ext[k], lo[k]);
            atomicMax(&ext[3 + k], hi[k]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool empty = begin >= end;
        const float inf = __builtin_inff();
        a.bounds[6 * s + threadIdx.x] = empty ? (threadIdx.x < 3 ? inf : -inf) : fr::voxel_centre(ext[threadIdx.x], a.voxel);
    }
}

}  // namespace vf
