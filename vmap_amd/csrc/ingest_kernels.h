// ingest_kernels.h - frame ingest on the device: what the reference's data loader does on the host per frame with one full-frame
// numpy pass per instance (dataset.py:87-133, image_transforms.py:13-33).  A decoded frame as the image files hold it (row-major
// [H, W]: rgb u8, depth u16 / f32, instance and class labels u16 / i32) becomes a FrameStore slot in store layout ([W, H]: rgbx,
// depth in metres, relabelled instances) and the table of the objects in it with their enlarged 2-D boxes.  The rules are
// ingest_rules.h's; the contract is the ingest section of include/vmapstep.h.
//
// Four launches on one stream, no host step between them; everything blocks combine is an integer sum, minimum or maximum, so the
// output is bit-identical from call to call:
//   ingest_init     every copy of the global table = the identity of every statistic (count 0, minima INT_MAX, maxima -1 / INT_MIN),
//                   overflow = 0
//   ingest_stats    reads inst and sem once, in [H, W] order, 64 consecutive pixels per wave, all of a lane's loads in flight before
//                   the first is used.  Neighbouring pixels share ids, so the wave combines first: the first pending lane's (id, row)
//                   is broadcast, the lanes that match are balloted, and that ONE lane carries the run - its count is the ballot's
//                   popcount, its u extent the first and last set bit (lanes of one row are consecutive columns), its v the row -
//                   until no lane is pending.  Runs meet in an LDS table keyed by id (kSlots slots, open addressing, kProbes probes,
//                   LDS atomics); a run that finds no slot goes to the global table directly.  At the end every used slot is flushed
//                   with seven integer atomics - into copy blockIdx % replicas of the table: the rows of the large instances are met
//                   by every workgroup, and the atomics of a whole grid on one address serialise.  A lane whose class differs from
//                   its run's leader sends its class to the global table itself (a mixed id is an error anyway).  Pixels whose id
//                   has no table row are counted into `overflow`.
//   ingest_decide   one workgroup: the copies of every row merged, ir::decide for it, the status column, and the present rows
//                   compacted in ascending id (scan_ops.h) behind the header (n_rows, overflow)
//   ingest_write    the transposing pass: a kTile x kTile tile is read along W (rgb packed to 4 bytes, depth converted, the label
//                   looked up in the status column - small and L2-resident), staged in LDS with rows padded by one word so that
//                   neither the row-wise store nor the column-wise load conflicts, and written along H into the slot
// 16-bit and 32-bit inputs are chosen by a wave-uniform branch on a flag of the argument block.
#pragma once
#include <hip/hip_runtime.h>

#include "ingest_rules.h"
#include "launch_geometry.h"
#include "scan_ops.h"

namespace vi {

struct IngestArgs {
    ir::Rules rules;
    int max_ids;
    int label_i32, depth_f32;              // input types: labels int32 (else uint16), depth float32 (else uint16)
    const unsigned char* rgb;              // [H][W][3]
    const void* depth;                     // [H][W]
    const void* inst;                      // [H][W] or null: no labels, every pixel is id 0 and stays 0
    const void* sem;                       // [H][W] or null: class 0 everywhere
    unsigned* out_rgbx;                    // [W][H] (r, g, b, 0)
    float* out_depth;                      // [W][H]
    int* out_inst;                         // [W][H]
    int* rows_out;                         // n_rows, overflow, then [n_rows][ir::kRowInts]
    int* overflow;                         // workspace
    int* table;                            // workspace: [replicas][max_ids][kTableInts]
    int replicas;
    int* status;                           // workspace: [max_ids]
    long long n_pix;
};

constexpr int kIntMax = 2147483647, kIntMin = -2147483647 - 1;

__device__ __forceinline__ int stat_identity(int field) {
    return field == 0 || field == 7 ? 0 : field == 1 || field == 3 || field == 5 ? kIntMax : field == 6 ? kIntMin : -1;
}

__device__ __forceinline__ int load_label(const void* p, long long i, int is_i32) {
    return is_i32 ? static_cast<const int*>(p)[i] : (int)static_cast<const unsigned short*>(p)[i];
}

// whether id has a table row (row = id + 1), without overflowing on any int32 id
__device__ __forceinline__ bool has_row(int id, int max_ids) { return id >= -1 && id <= max_ids - 2; }

// one run (or one flushed slot) into a row of statistics, in LDS or in global memory
__device__ __forceinline__ void accumulate(int* dst, int count, int u_lo, int u_hi, int v_lo, int v_hi, int c_lo, int c_hi) {
    atomicAdd(dst + 0, count);
    atomicMin(dst + 1, u_lo);
    atomicMax(dst + 2, u_hi);
    atomicMin(dst + 3, v_lo);
    atomicMax(dst + 4, v_hi);
    atomicMin(dst + 5, c_lo);
    atomicMax(dst + 6, c_hi);
}

__global__ void __launch_bounds__(kIngestWG) ingest_init(IngestArgs a) {
    const int i = blockIdx.x * kIngestWG + threadIdx.x;
    if (i < a.replicas * a.max_ids * kTableInts) a.table[i] = stat_identity(i & (kTableInts - 1));
    if (i == 0) *a.overflow = 0;
}

__global__ void __launch_bounds__(kIngestWG) ingest_stats(IngestArgs a) {
    __shared__ int key[kSlots];
    __shared__ int acc[kSlots][kTableInts];
    __shared__ int ovf;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < kSlots) {
        key[tid] = -1;
#pragma unroll
        for (int f = 0; f < kTableInts; ++f) acc[tid][f] = stat_identity(f);
    }
    if (tid == 0) ovf = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kStatsPix;
    const int W = a.rules.width;
    int* const table = a.table + (long long)(blockIdx.x % a.replicas) * a.max_ids * kTableInts;     // this workgroup's copy
    int ids[kStatsPer], classes[kStatsPer];
#pragma unroll
    for (int it = 0; it < kStatsPer; ++it) {                  // every load of the lane is in flight before the first is used
        const long long p = base + it * kIngestWG + tid;
        ids[it] = classes[it] = 0;
        if (p < a.n_pix) {
            if (a.inst) ids[it] = load_label(a.inst, p, a.label_i32);
            if (a.sem) classes[it] = load_label(a.sem, p, a.label_i32);
        }
    }
#pragma unroll
    for (int it = 0; it < kStatsPer; ++it) {
        const long long p = base + it * kIngestWG + tid;
        const bool active = p < a.n_pix;
        const int id = ids[it], cls = classes[it];
        int u = 0, v = 0;
        if (active) {
            v = (int)(p / W);
            u = (int)(p - (long long)v * W);
        }
        const bool counted = active && has_row(id, a.max_ids);
        const int row = counted ? id + 1 : 0;
        const unsigned long long lost = __ballot(active && !counted);
        if (lost != 0 && lane == 0) atomicAdd(&ovf, __popcll(lost));
        unsigned long long todo = __ballot(counted);
        while (todo != 0) {                                   // wave-uniform: one round per (id, image row) among the wave's pixels
            const int leader = __ffsll((long long)todo) - 1;
            const int lrow = __shfl(row, leader, 64), lv = __shfl(v, leader, 64), lcls = __shfl(cls, leader, 64);
            const bool mine = counted && row == lrow && v == lv;
            const unsigned long long m = __ballot(mine);
            if (mine && cls != lcls) {                        // a second class on the id: rare, and an error for the caller
                atomicMin(table + (long long)row * kTableInts + 5, cls);
                atomicMax(table + (long long)row * kTableInts + 6, cls);
            }
            if (lane == leader) {
                const int count = __popcll(m), u_hi = u + (63 - __clzll((long long)m)) - leader;
                int slot = -1;
                for (int k = 0; k < kProbes && slot < 0; ++k) {
                    const int s = (row + k) & (kSlots - 1);
                    const int prev = atomicCAS(&key[s], -1, row);
                    if (prev == -1 || prev == row) slot = s;
                }
                if (slot >= 0) accumulate(acc[slot], count, u, u_hi, v, v, cls, cls);
                else accumulate(table + (long long)row * kTableInts, count, u, u_hi, v, v, cls, cls);
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

__global__ void __launch_bounds__(kDecideWG) ingest_decide(IngestArgs a) {
    __shared__ int wsum[kDecideWG / 64];
    // the copies of a row merged: sums of the counts, extremes of the extremes (a row is two 16-byte loads)
    auto merged = [&](long long r) {
        ir::Stats s;
        s.count = 0; s.u_min = s.v_min = s.c_min = kIntMax; s.u_max = s.v_max = -1; s.c_max = kIntMin;
        for (int k = 0; k < a.replicas; ++k) {
            const int4* t = reinterpret_cast<const int4*>(a.table + ((long long)k * a.max_ids + r) * kTableInts);
            const int4 lo = t[0], hi = t[1];
            s.count += lo.x;
            s.u_min = min(s.u_min, lo.y); s.u_max = max(s.u_max, lo.z);
            s.v_min = min(s.v_min, lo.w); s.v_max = max(s.v_max, hi.x);
            s.c_min = min(s.c_min, hi.y); s.c_max = max(s.c_max, hi.z);
        }
        return s;
    };
    ir::Stats s;                                              // of the row this lane holds in the current chunk: read once, in load
    // id 0 (row 1) is always reported, with the full-frame box
    const int n = vscan::wg_scan_totals<kDecideWG, int>(a.max_ids, wsum, [&](long long r) -> int {
        s = merged(r);
        return r == 1 || s.count > 0 ? 1 : 0;
    }, [&](long long r, int pos) {
        const int id = (int)r - 1;
        const ir::Decision d = ir::decide(a.rules, id, s);
        a.status[r] = d.status;
        if (r == 1 || s.count > 0) {
            int* o = a.rows_out + 2 + (long long)pos * ir::kRowInts;
            o[0] = id; o[1] = d.status; o[2] = s.count;
            o[3] = d.box[0]; o[4] = d.box[1]; o[5] = d.box[2]; o[6] = d.box[3];
            o[7] = d.cls;
        }
    });
    if (threadIdx.x == 0) {
        a.rows_out[0] = n;
        a.rows_out[1] = *a.overflow;
    }
}

__global__ void __launch_bounds__(kIngestWG) ingest_write(IngestArgs a) {
    __shared__ unsigned tile[3][kTile][kTile + 1];
    const int W = a.rules.width, H = a.rules.height;
    const int u0 = blockIdx.x * kTile, v0 = blockIdx.y * kTile;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int kRounds = kTile / (kIngestWG / 64);
#pragma unroll 4
    for (int j = 0; j < kRounds; ++j) {                       // a wave reads 64 consecutive columns of one row
        const int vo = w + j * (kIngestWG / 64), u = u0 + lane, v = v0 + vo;
        if (u < W && v < H) {
            const long long p = (long long)v * W + u;
            const unsigned char* c = a.rgb + p * 3;
            const unsigned px = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
            const float raw = a.depth_f32 ? static_cast<const float*>(a.depth)[p] : (float)static_cast<const unsigned short*>(a.depth)[p];
            int lab = 0;
            if (a.inst) {
                const int id = load_label(a.inst, p, a.label_i32);
                if (has_row(id, a.max_ids)) lab = ir::label_of(id, a.status[id + 1]);
            }
            tile[0][vo][lane] = px;
            tile[1][vo][lane] = __float_as_uint(ir::depth_of(raw, a.rules.depth_scale, a.rules.max_depth));
            tile[2][vo][lane] = (unsigned)lab;
        }
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < kRounds; ++j) {                       // a wave writes 64 consecutive rows of one column
        const int uo = w + j * (kIngestWG / 64), u = u0 + uo, v = v0 + lane;
        if (u < W && v < H) {
            const long long q = (long long)u * H + v;
            a.out_rgbx[q] = tile[0][lane][uo];
            a.out_depth[q] = __uint_as_float(tile[1][lane][uo]);
            a.out_inst[q] = (int)tile[2][lane][uo];
        }
    }
}

}  // namespace vi
