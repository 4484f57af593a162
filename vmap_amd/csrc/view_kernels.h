// view_kernels.h - view rendering: every object field composited per pixel of a camera image (no counterpart in the reference, whose
// vis.py only meshes; built from its ray convention vmap.py:31-41 / 507-516, its point arithmetic vmap.py:452-454 and its compositing
// render_rays.py:26-51).
//
//   view_count      one lane per pixel of the call's pixel range, blocks of kViewBlock = 64 pixels = one wave.  Per object the lanes
//                   whose ray crosses the object's box (view_geometry.h: vg::box_segment) are counted by a ballot: one total per
//                   (object, block)
//   view_scan       one workgroup: exclusive scan of the totals in (object, block) order (scan_ops.h) -> the pair offsets per object
//   view_emit       the same hit test; rank inside the block from the ballot; one 16-byte pair record (pixel, t_near, dt, 0) per hit,
//                   ordered by (object, pixel)
//   view_plan       one workgroup: the launch plan of field_query_seg_s32 (query_split_kernels.h, the hot kernel: the field at every
//                   sample of every pair) from the device offsets, by the formula of vl::scene_plan_host
//   view_composite  one lane per pixel: the hit test a third time, the pair index from block prefix + ballot rank, at most
//                   kViewMaxHits (t_near, dt, sample base, cursor) entries in LDS, merged by repeatedly taking the smallest (t, object)
// Objects come in up to kViewMaxGroups field groups with their own hidden width and samples per hit (ViewArgs::g_*): the kernels here
// walk group after group, and the field pass is one field kernel launch per group - field_query_seg_s32 at hidden 32,
// field_query_seg_gen<NB> (query_kernels.h) at the wider widths.  A view of one group is the case g_end = {n, n, n, n}.
// The three passes call ONE inline function (view_hit), so they cannot disagree on a hit; nothing blocks combine is a float sum, so the
// images are bit-identical from call to call and for any split of the pixel range into calls.
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "scan_ops.h"
#include "view_args.h"

namespace vv {

static_assert(kViewMaxHits == vg::kMaxHits, "one cap");

// this lane's pixel and ray: live = the pixel lies in the call's range
__device__ __forceinline__ bool view_lane(const ViewArgs& a, long long& pix, vg::Ray& r) {
    pix = a.pix_begin + (long long)blockIdx.x * kViewBlock + threadIdx.x;
    const bool live = pix < a.pix_end;
    const long long p = live ? pix : a.pix_begin;
    r = vg::pixel_ray(a.cam, (int)(p / a.cam.height), (int)(p % a.cam.height));
    return live;
}

// THE hit test of all three passes (S = the sample count of the object's group)
__device__ __forceinline__ bool view_hit(const ViewArgs& a, const vg::Ray& r, bool live, int k, int S, float& t_near, float& dt) {
    const bool hit = vg::box_segment(r, a.boxes + 15 * k, a.cam.min_depth, S, t_near, dt);
    return live && hit;
}

__device__ __forceinline__ int ballot_rank(unsigned long long ballot) {
    return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// The three passes walk the objects group after group - `for (int g = 0, k = 0; g < kViewMaxGroups; ++g) for (; k < g_end[g]; ++k)` -
// so that the group's sample count, sample shift and end are loop invariants (the groups past the last one are empty: g_end = n_obj).

__global__ void __launch_bounds__(kViewBlock) view_count(const ViewArgs a) {
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    for (int g = 0, k = 0; g < kViewMaxGroups; ++g) {
        const int S = a.g_samples[g], end = a.g_end[g];
        for (; k < end; ++k) {
            float tn, dt;
            const unsigned long long b = __ballot(view_hit(a, r, live, k, S, tn, dt));
            if (threadIdx.x == 0) a.blk[(long long)k * a.nb + blockIdx.x] = __popcll(b);
        }
    }
}

__global__ void __launch_bounds__(kViewScanWG) view_scan(const ViewArgs a) {
    __shared__ long long wsum[kViewScanWG / 64];
    const long long n = (long long)a.n_obj * a.nb;
    const long long carry = vscan::wg_scan_totals<kViewScanWG>(
        n, wsum, [&](long long b) { return a.blk[b]; }, [&](long long b, long long ex) { a.blk[b] = ex; });
    __syncthreads();                           // the offsets below read prefixes other lanes stored
    for (int o = threadIdx.x; o <= a.n_obj; o += kViewScanWG) a.offsets[o] = o < a.n_obj ? a.blk[(long long)o * a.nb] : carry;
}

__global__ void __launch_bounds__(kViewBlock) view_emit(const ViewArgs a) {
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    for (int g = 0, k = 0; g < kViewMaxGroups; ++g) {
        const int S = a.g_samples[g], end = a.g_end[g];
        for (; k < end; ++k) {
            float tn, dt;
            const bool hit = view_hit(a, r, live, k, S, tn, dt);
            const long long at = a.blk[(long long)k * a.nb + blockIdx.x] + ballot_rank(__ballot(hit));
            if (hit && at >= 0 && at < a.cap) a.pairs[at] = vg::Pair{(int)pix, tn, dt, 0};
        }
    }
}

// one lane per object; an entry holds the object's index inside its group (the field kernel of a group sees its objects alone) and
// the group's chunks per entry; entries come out in object order, so a group's entries are contiguous
__global__ void __launch_bounds__(kViewPlanWG) view_plan(const ViewArgs a) {
    __shared__ int wsum[kViewPlanWG / 64];
    const int k = threadIdx.x;
    int g = 0;
#pragma unroll
    for (int i = 0; i < kViewMaxGroups - 1; ++i) g += k < a.n_obj && k >= a.g_end[i] ? 1 : 0;
    const long long per = a.g_per[g];
    const int kg = g > 0 ? k - a.g_end[g - 1] : k;
    long long chunks = 0;
    if (k < a.n_obj) chunks = ((a.offsets[k + 1] - a.offsets[k]) * a.g_samples[g] + kViewChunk - 1) / kViewChunk;
    const int mine = (int)((chunks + per - 1) / per);
    int total;
    const int first = vscan::wg_exclusive_scan<kViewPlanWG>(mine, wsum, total);
    for (int e = 0; e < mine && first + e < a.plan_cap; ++e) {
        const long long c0 = e * per, c1 = c0 + per < chunks ? c0 + per : chunks;
        int* q = a.plan + 4 * (first + e);
        q[0] = kg; q[1] = (int)c0; q[2] = (int)c1; q[3] = 0;
    }
}

// The one kernel with two instantiations (every single-form build of it measured 4-5 % slower on the one-group view).
// GROUPS: an entry's object and its group's sample count share one LDS word, e_obj = object << 8 | S (S <= kViewMaxSamples < 2^8) -
// six arrays, 24 KiB per workgroup, six workgroups per compute unit; a pixel holds an object once, so the words order as the objects
// do and the (t, object) comparisons take them as they are.  !GROUPS (a view of one group, g_end[0] = n_obj): one flat object loop,
// the uniform cam.samples, e_obj = object.
static_assert(kViewMaxSamples < 256, "entry word: sample count in bits 0-7, object above");

template <bool GROUPS>
__global__ void __launch_bounds__(kViewBlock) view_composite(const ViewArgs a) {
    __shared__ float e_tn[kViewMaxHits][kViewBlock], e_dt[kViewMaxHits][kViewBlock], e_w[kViewMaxHits][kViewBlock];
    __shared__ int e_base[kViewMaxHits][kViewBlock], e_cur[kViewMaxHits][kViewBlock], e_obj[kViewMaxHits][kViewBlock];
    const int lane = threadIdx.x;
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    int n = 0;
    bool over = false;
    auto object = [&](int k, int S, long long shift) {
        float tn, dt;
        const bool hit = view_hit(a, r, live, k, S, tn, dt);
        const long long at = a.blk[(long long)k * a.nb + blockIdx.x] + ballot_rank(__ballot(hit));
        // a pair index outside the object's segment (or the buffers) is never dereferenced
        if (hit && at >= a.offsets[k] && at < a.offsets[k + 1] && at < a.cap) {
            int slot = n;
            if (n == kViewMaxHits) {
                // more boxes than the cap: the kViewMaxHits smallest by (t_near, object) stay.  k exceeds every kept object, so the
                // new hit replaces the largest kept one only where its t_near is strictly smaller
                over = true;
                int worst = 0;
                for (int e = 1; e < kViewMaxHits; ++e) {
                    const bool more = e_tn[e][lane] > e_tn[worst][lane] || (e_tn[e][lane] == e_tn[worst][lane] && e_obj[e][lane] > e_obj[worst][lane]);
                    worst = more ? e : worst;
                }
                slot = tn < e_tn[worst][lane] ? worst : -1;
            } else {
                ++n;
            }
            if (slot >= 0) {
                e_tn[slot][lane] = tn; e_dt[slot][lane] = dt; e_w[slot][lane] = 0.0f;
                e_base[slot][lane] = (int)(at * S + shift);
                e_cur[slot][lane] = 0; e_obj[slot][lane] = GROUPS ? k << 8 | S : k;
            }
        }
    };
    if constexpr (GROUPS) {
        for (int g = 0, k = 0; g < kViewMaxGroups; ++g) {
            const int S = a.g_samples[g], end = a.g_end[g];
            const long long shift = a.g_shift[g];
            for (; k < end; ++k) object(k, S, shift);
        }
    } else {
        for (int k = 0; k < a.n_obj; ++k) object(k, a.cam.samples, 0);
    }
    if (!live) return;
    if (over) atomicAdd(a.overflow, 1);
    float depth = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, opacity = 0.0f, T = 1.0f;
    {
#pragma clang fp contract(off)
        for (;;) {
            int best = -1, bobj = 0;
            float bt = 0.0f;
            for (int e = 0; e < n; ++e) {
                const int o = e_obj[e][lane];
                if (e_cur[e][lane] >= (GROUPS ? o & 255 : a.cam.samples)) continue;
                const float t = vg::sample_depth(e_tn[e][lane], e_dt[e][lane], e_cur[e][lane]);
                if (best < 0 || t < bt || (t == bt && o < bobj)) { best = e; bt = t; bobj = o; }
            }
            if (best < 0) break;
            const long long at = (long long)e_base[best][lane] + e_cur[best][lane];
            e_cur[best][lane] += 1;
            const float occ = a.occ[at];
            const float w = occ * T;                         // render_rays.py:34  occupancy * cumprod(free_probs)
            T = T * ((1.0f - occ) + 1e-10f);                 // render_rays.py:32  1. - occupancy + 1e-10
            depth = depth + w * bt;                          // render_rays.py:47-49
            c0 = c0 + w * a.rgb[3 * at];
            c1 = c1 + w * a.rgb[3 * at + 1];
            c2 = c2 + w * a.rgb[3 * at + 2];
            opacity = opacity + w;
            e_w[best][lane] = e_w[best][lane] + w;
        }
    }
    int inst = -1;
    float wbest = 0.0f;
    for (int e = 0; e < n; ++e) {
        const float w = e_w[e][lane];
        const int o = GROUPS ? e_obj[e][lane] >> 8 : e_obj[e][lane];
        if (inst < 0 || w > wbest || (w == wbest && o < inst)) { inst = o; wbest = w; }
    }
    a.depth[pix] = depth;
    a.color[3 * pix] = c0; a.color[3 * pix + 1] = c1; a.color[3 * pix + 2] = c2;
    a.opacity[pix] = opacity;
    a.instance[pix] = inst;
}

}  // namespace vv
