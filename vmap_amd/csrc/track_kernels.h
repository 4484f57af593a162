// track_kernels.h - the instance tracker on the device: what the reference's track_instance (utils.py:274-382) does on the host per
// frame with several full-frame passes per detector mask (cv2.erode, two Open3D unprojections, the inside test against every known
// instance of the mask's class).  A decoded frame (row-major [H, W]: depth u16 / f32, the detector's label image u16 / i32), the pose,
// the class of every detection row, the frame's pair table (per row the known instances of its class, ascending) and the table of
// the boxes registered so far become the per-row table (statistics, status, persistent id), the inside count of every pair, the voxel
// keys that join the instances' clouds and the label image of persistent ids.  The rules are track_rules.h's and, through it,
// filter_rules.h's; the contract is the track section of include/vmapstep.h.
//
// Everything blocks combine is an integer sum and keys are written in pixel order, so the output is bit-identical from call to call:
//   track_init      every copy of the two global tables = 0, overflow = 0
//   track_stats     filter_stats' tile, halo and erosion passes on the detection rows.  A wave owns 64 consecutive columns of one
//                   row; the first pending lane's detection is broadcast and the lanes that match are balloted.  Inside that
//                   wave-uniform round the wave walks the detection's candidates: every lane has computed its world point once,
//                   the candidate's box row is read at a wave-uniform address, the pair's count is the popcount of a ballot, and
//                   the leader adds it to an LDS table keyed by pair index (vt::kPairSlots slots, open addressing; no slot: the
//                   global table directly).  The row's own counts go to an LDS table keyed by row, as the filter's.  Used slots are
//                   flushed with integer atomics into copy (block % kReplicas) of the global tables.  No lane waits on another
//                   workgroup and every loop is bounded by a count fixed before the launch (the tile, the probes, the pair table)
//   track_decide    one workgroup: the copies of the pair table summed into copy 0, then per row the copies of its statistics merged,
//                   tr::decide, the NEW rows numbered and the present rows compacted by one scan (both counts in one 64-bit word),
//                   the status and id columns and the inside counts of the pairs behind the rows
//   track_count / track_scan / track_emit   the filter's count -> scan -> emit key path through the status and id columns: a NEW
//                   row's valid eroded pixels under its new id, a MERGED row's valid pixels inside the matched instance's old box
//                   (recomputed) under that instance's id
//   track_write     the label image: tr::label_of by the two columns, the inside test recomputed in the same way
// The loads are the filter's own (filter_loads.h), on a FilterArgs filled from the fields they read.
#pragma once
#include <hip/hip_runtime.h>

#include "filter_loads.h"
#include "launch_geometry.h"
#include "scan_ops.h"
#include "track_rules.h"

namespace vt {

using vf::kDecideWG;
using vf::kFilterWG;
using vf::kHaloH;
using vf::kHaloW;
using vf::kPixPer;
using vf::kReplicas;
using vf::kSlots;
using vf::kTileH;
using vf::kTileW;

struct TrackArgs {
    tr::Rules rules;
    int label_i32, depth_f32;              // input types: the label image int32 (else uint16), depth float32 (else uint16)
    int vec_ok;                            // depth, det and labels_out are 16-byte aligned
    int max_pairs, n_pairs;
    const void* depth;                     // [H][W]
    const void* det;                       // [H][W]
    const int* det_class;                  // [max_det]
    const int* pair_off;                   // [max_det + 1]: row d's candidates are pairs [pair_off[d], pair_off[d + 1])
    const int* pair_inst;                  // [max_pairs]: a persistent id
    const float* box_table;                // [max_ids][fr::kBoxFloats]
    int* status;                           // [max_det]
    int* ident;                            // [max_det]: the persistent id of a NEW or MERGED row, else 0
    int* rows_out;                         // tr::kHeadInts, then [max_det][tr::kRowInts], then [max_pairs] inside counts
    unsigned long long* keys_out;          // [n_pix]
    int* labels_out;                       // [H][W]
    int* overflow;                         // workspace
    int* table;                            // workspace: [kReplicas][max_det][kStatInts]
    int* pairs;                            // workspace: [kReplicas][max_pairs]
    unsigned char* flags;                  // workspace: [n_pix]
    int* blk;                              // workspace: [n_blk][2]
    int n_blk;
    long long n_pix;
};

// what filter_loads.h's vector loads read of their argument block
__device__ __forceinline__ vf::FilterArgs loads_of(const TrackArgs& a) {
    vf::FilterArgs f = {};
    f.label_i32 = a.label_i32; f.depth_f32 = a.depth_f32; f.vec_ok = a.vec_ok; f.depth = a.depth; f.n_pix = a.n_pix;
    return f;
}

__device__ __forceinline__ int row_of(const TrackArgs& a, int raw) { return fr::shifted_id(raw, a.rules.frame.id_shift, a.rules.frame.max_ids); }

// the candidates of row d, clipped to the pair table
__device__ __forceinline__ void pairs_of(const TrackArgs& a, int d, int& p0, int& p1) {
    p0 = max(a.pair_off[d], 0);
    p1 = min(a.pair_off[d + 1], a.n_pairs);
}

__global__ void __launch_bounds__(kFilterWG) track_init(TrackArgs a) {
    const long long i = (long long)blockIdx.x * kFilterWG + threadIdx.x;
    if (i < (long long)kReplicas * a.rules.frame.max_ids * kStatInts) a.table[i] = 0;
    if (i < (long long)kReplicas * a.max_pairs) a.pairs[i] = 0;
    if (i == 0) *a.overflow = 0;
}

__global__ void __launch_bounds__(kFilterWG) track_stats(TrackArgs a) {
    __shared__ int ids[kHaloH][kHaloW + 1];
    __shared__ unsigned char rowrun[kHaloH][kTileW];
    __shared__ int key[kSlots];
    __shared__ int acc[kSlots][kStatInts];
    __shared__ int pkey[kPairSlots];
    __shared__ int pacc[kPairSlots];
    __shared__ int ovf;
    const fr::Rules& fr_ = a.rules.frame;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = fr_.width, H = fr_.height, r = fr_.erode_radius, max_det = fr_.max_ids;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int hw = kTileW + 2 * r, hh = kTileH + 2 * r;       // <= kHaloW, kHaloH: r <= kMaxRadius is checked before the launch
    if (tid < kSlots) {
        key[tid] = -1;
#pragma unroll
        for (int f = 0; f < kStatInts; ++f) acc[tid][f] = 0;
    }
    if (tid < kPairSlots) {
        pkey[tid] = -1;
        pacc[tid] = 0;
    }
    if (tid == 0) ovf = 0;
    for (int i = tid; i < hw * hh; i += kFilterWG) {          // the tile and its halo: the detection row, -1 or -2
        const int hy = i / hw, hx = i - hy * hw;
        const int y = y0 - r + hy, x = x0 - r + hx;
        int v = -2;
        if (x >= 0 && x < W && y >= 0 && y < H) v = row_of(a, vf::load_label(a.det, (long long)y * W + x, a.label_i32));
        ids[hy][hx] = v;
    }
    __syncthreads();
    for (int i = tid; i < hh * kTileW; i += kFilterWG) {      // the row pass: the in-image cells of the row window carry the cell's row
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
    const long long replica = (blockIdx.y * gridDim.x + blockIdx.x) % kReplicas;
    int* const table = a.table + replica * max_det * kStatInts;
    int* const pairs = a.pairs + replica * a.max_pairs;
    constexpr int kRounds = kTileH / (kFilterWG / 64);
    for (int j = 0; j < kRounds; ++j) {                       // a wave owns 64 consecutive columns of one row
        const int ty = wave + j * (kFilterWG / 64), x = x0 + lane, y = y0 + ty;
        const bool active = x < W && y < H;
        const int d = ids[ty + r][lane + r];                  // -2 exactly where !active
        bool eroded = true;
        for (int dy = 0; dy <= 2 * r; ++dy) {                 // the column pass
            const int v = ids[ty + dy][lane + r];
            eroded = eroded && (v == -2 || (v == d && rowrun[ty + dy][lane] != 0));
        }
        bool valid = false;
        fr::Point pt = {0.0f, 0.0f, 0.0f};
        if (active) {
            const long long p = (long long)y * W + x;
            const float depth = ir::depth_of(vf::load_depth(a.depth, p, a.depth_f32), fr_.depth_scale, fr_.max_depth);
            valid = fr::valid_depth(depth);
            if (valid) pt = fr::world_point(fr_.cam, x, y, depth);                 // once, for every candidate
            a.flags[p] = (unsigned char)((valid ? fr::VALID : 0) | (eroded ? fr::ERODED : 0));
        }
        const bool counted = active && d >= 0;
        const unsigned long long lost = __ballot(active && d == -1);
        if (lost != 0 && lane == 0) atomicAdd(&ovf, __popcll(lost));
        unsigned long long todo = __ballot(counted);
        while (todo != 0) {                                   // wave-uniform: one round per detection among the wave's pixels
            const int leader = __ffsll((long long)todo) - 1;
            const int ld = __builtin_amdgcn_readfirstlane(__shfl(d, leader, 64));
            const bool mine = counted && d == ld;
            const unsigned long long m = __ballot(mine);
            const int n_valid = __popcll(__ballot(mine && valid));
            const int n_eroded = __popcll(__ballot(mine && eroded)), n_ev = __popcll(__ballot(mine && eroded && valid));
            if (lane == leader) {
                int slot = -1;
                for (int k = 0; k < vf::kProbes && slot < 0; ++k) {
                    const int s = (ld + k) & (kSlots - 1);
                    const int prev = atomicCAS(&key[s], -1, ld);
                    if (prev == -1 || prev == ld) slot = s;
                }
                int* dst = slot >= 0 ? acc[slot] : table + (long long)ld * kStatInts;
                atomicAdd(dst + 0, __popcll(m));
                if (n_valid) atomicAdd(dst + 1, n_valid);
                if (n_eroded) atomicAdd(dst + 2, n_eroded);
                if (n_ev) atomicAdd(dst + 3, n_ev);
            }
            if (n_valid != 0) {                               // the candidates of the detection, wave-uniform
                int p0, p1;
                pairs_of(a, ld, p0, p1);
                for (int p = p0; p < p1; ++p) {
                    const int inst = a.pair_inst[p];
                    if (inst < 0 || inst >= a.rules.max_ids) continue;
                    const float* row = a.box_table + (long long)inst * fr::kBoxFloats;
                    const int c = __popcll(__ballot(mine && valid && fr::inside_box(row, pt)));
                    if (lane == leader) {                     // every pair the workgroup sees takes a slot, a count of 0 included
                        int slot = -1;
                        for (int k = 0; k < kPairProbes && slot < 0; ++k) {
                            const int s = (p + k) & (kPairSlots - 1);
                            const int prev = atomicCAS(&pkey[s], -1, p);
                            if (prev == -1 || prev == p) slot = s;
                        }
                        if (c != 0) atomicAdd(slot >= 0 ? &pacc[slot] : pairs + p, c);
                    }
                }
            }
            todo &= ~m;
        }
    }
    __syncthreads();
    if (tid < kSlots && key[tid] >= 0) {
        int* dst = table + (long long)key[tid] * kStatInts;
#pragma unroll
        for (int f = 0; f < kStatInts; ++f)
            if (acc[tid][f]) atomicAdd(dst + f, acc[tid][f]);
    }
    if (tid < kPairSlots && pkey[tid] >= 0 && pacc[tid] != 0) atomicAdd(pairs + pkey[tid], pacc[tid]);
    if (tid == 0 && ovf != 0) atomicAdd(a.overflow, ovf);
}

__global__ void __launch_bounds__(kDecideWG) track_decide(TrackArgs a) {
    __shared__ long long wsum[kDecideWG / 64];
    const int max_det = a.rules.frame.max_ids;
    int* const inside = a.rows_out + tr::kHeadInts + (long long)max_det * tr::kRowInts;      // the summed pair table, for the host too
    for (int p = threadIdx.x; p < a.n_pairs; p += kDecideWG) {
        int s = 0;
        for (int k = 0; k < kReplicas; ++k) s += a.pairs[(long long)k * a.max_pairs + p];
        inside[p] = s;
    }
    __syncthreads();
    tr::Stats s;                                              // of the row this lane holds in the current chunk
    int st = 0, match = -1, cls = 0, p0 = 0;
    const long long n = vscan::wg_scan_totals<kDecideWG, long long>(max_det, wsum, [&](long long r) -> long long {
        int4 t = make_int4(0, 0, 0, 0);
        for (int k = 0; k < kReplicas; ++k) {
            const int4 v = *reinterpret_cast<const int4*>(a.table + ((long long)k * max_det + r) * kStatInts);
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        s.pixels = t.x; s.valid = t.y; s.eroded = t.z; s.eroded_valid = t.w;
        int p1;
        pairs_of(a, (int)r, p0, p1);
        cls = r < a.rules.n_det ? a.det_class[r] : 0;
        st = tr::decide(a.rules, (int)r, cls, s, inside + p0, max(p1 - p0, 0), &match);
        return (s.pixels > 0 ? 1ll : 0ll) | (st == tr::NEW ? 1ll << 32 : 0ll);
    }, [&](long long r, long long before) {
        const int pos = (int)(before & 0xffffffffll), rank = (int)(before >> 32);
        const int id = st == tr::NEW ? a.rules.next_id + rank : st == tr::MERGED ? a.pair_inst[p0 + match] : 0;
        a.status[r] = st;
        a.ident[r] = id;
        if (s.pixels > 0) {
            int* o = a.rows_out + tr::kHeadInts + (long long)pos * tr::kRowInts;
            o[0] = (int)r; o[1] = st; o[2] = cls; o[3] = id; o[4] = s.pixels;
            o[5] = s.valid; o[6] = st == tr::MERGED ? inside[p0 + match] : 0; o[7] = s.eroded; o[8] = s.eroded_valid;
        }
    });
    if (threadIdx.x == 0) {
        a.rows_out[0] = (int)(n & 0xffffffffll);
        a.rows_out[1] = *a.overflow;
        a.rows_out[2] = 0;
        a.rows_out[3] = 0;
    }
}

// whether the pixel's point lies inside the box the matched instance had when the frame arrived (a MERGED row's valid pixel)
__device__ __forceinline__ bool inside_old(const TrackArgs& a, int id, long long p, float depth) {
    if (id < 0 || id >= a.rules.max_ids) return false;
    const int W = a.rules.frame.width;
    const int v = (int)(p / W), u = (int)(p - (long long)v * W);
    return fr::inside_box(a.box_table + (long long)id * fr::kBoxFloats, fr::world_point(a.rules.frame.cam, u, v, depth));
}

// the keys of this lane's pixels (bit c of the result: pixel c emits keys[c]); out: its points outside the grid
__device__ __forceinline__ int emit_lane(const TrackArgs& a, long long pix0, unsigned long long (&keys)[kPixPer], int& out) {
    int raw[kPixPer];
    float depth[kPixPer];
    out = 0;
    if (pix0 >= a.n_pix) return 0;
    const vf::FilterArgs f = loads_of(a);
    vf::load_labels4(f, a.det, pix0, raw);
    vf::load_depths4(f, pix0, depth);
    const int W = a.rules.frame.width;
    int mask = 0;
#pragma unroll
    for (int c = 0; c < kPixPer; ++c) {
        const long long p = pix0 + c;
        if (p >= a.n_pix) break;
        const int d = row_of(a, raw[c]);
        if (d < 0) continue;
        const int st = a.status[d];
        if (st != tr::NEW && st != tr::MERGED) continue;
        const int id = a.ident[d];
        int flags = a.flags[p];
        if (!(flags & fr::VALID)) continue;
        const float dep = ir::depth_of(depth[c], a.rules.frame.depth_scale, a.rules.frame.max_depth);
        if (st == tr::MERGED && inside_old(a, id, p, dep)) flags |= fr::INSIDE;
        if (!tr::emits(st, flags)) continue;
        const int v = (int)(p / W), u = (int)(p - (long long)v * W);
        if (fr::voxel_key(id, fr::world_point(a.rules.frame.cam, u, v, dep), a.rules.frame.voxel, &keys[c])) mask |= 1 << c;
        else ++out;
    }
    return mask;
}

__global__ void __launch_bounds__(kFilterWG) track_count(TrackArgs a) {
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

__global__ void __launch_bounds__(kDecideWG) track_scan(TrackArgs a) {
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

__global__ void __launch_bounds__(kFilterWG) track_emit(TrackArgs a) {
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

__global__ void __launch_bounds__(kFilterWG) track_write(TrackArgs a) {
    const long long pix0 = ((long long)blockIdx.x * kFilterWG + threadIdx.x) * kPixPer;
    if (pix0 >= a.n_pix) return;
    int raw[kPixPer], lab[kPixPer];
    float depth[kPixPer];
    const vf::FilterArgs f = loads_of(a);
    vf::load_labels4(f, a.det, pix0, raw);
    vf::load_depths4(f, pix0, depth);
#pragma unroll
    for (int c = 0; c < kPixPer; ++c) {
        const long long p = pix0 + c;
        lab[c] = 0;
        if (p >= a.n_pix) break;
        const int d = row_of(a, raw[c]);
        if (d < 0) continue;
        const int st = a.status[d], id = a.ident[d];
        bool valid = false, inside = false;
        if (st == tr::MERGED) {                               // against the box the matched instance had when the frame arrived
            const float dep = ir::depth_of(depth[c], a.rules.frame.depth_scale, a.rules.frame.max_depth);
            valid = fr::valid_depth(dep);
            inside = valid && inside_old(a, id, p, dep);
        }
        lab[c] = tr::label_of(id, st, valid, inside);
    }
    if (a.vec_ok && pix0 + kPixPer <= a.n_pix) {
        *reinterpret_cast<int4*>(a.labels_out + pix0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
    } else {
#pragma unroll
        for (int c = 0; c < kPixPer; ++c)
            if (pix0 + c < a.n_pix) a.labels_out[pix0 + c] = lab[c];
    }
}

}  // namespace vt
