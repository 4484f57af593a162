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
//                   sample of every pair) from the device offsets, by the formula of vl::view_plan_host
//   view_composite  one lane per pixel: the hit test a third time, the pair index from block prefix + ballot rank, at most
//                   kViewMaxHits (t_near, dt, sample base, cursor) entries in LDS, merged by repeatedly taking the smallest (t, object)
// A scene of several field groups (own hidden width and samples per hit each) runs the scene_view_* forms of the same bodies and one
// field kernel launch per group: field_query_seg_s32 at hidden 32, field_query_seg_gen<NB> (query_kernels.h) at the wider widths.
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

// The kernels exist in two forms with ONE body each (the template argument is a compile-time switch, so the single-group form is
// the code it was): the single-group form (one sample count, cam.samples) and the SCENE form (field groups, ViewArgs::g_*: an object's
// sample count is its group's, a pair's samples start at pair * S_g + g_shift[g]).
template <bool SCENE>
__device__ __forceinline__ int obj_group(const ViewArgs& a, int k) {
    if constexpr (!SCENE) return 0;
    int g = 0;
#pragma unroll
    for (int i = 0; i < kViewMaxGroups - 1; ++i) g += k >= a.g_end[i] ? 1 : 0;
    return g;
}
template <bool SCENE>
__device__ __forceinline__ int obj_samples(const ViewArgs& a, int k) {
    if constexpr (SCENE) return a.g_samples[obj_group<true>(a, k)];
    return a.cam.samples;
}

// THE hit test of all three passes (S = the object's sample count)
__device__ __forceinline__ bool view_hit(const ViewArgs& a, const vg::Ray& r, bool live, int k, int S, float& t_near, float& dt) {
    const bool hit = vg::box_segment(r, a.boxes + 15 * k, a.cam.min_depth, S, t_near, dt);
    return live && hit;
}

__device__ __forceinline__ int ballot_rank(unsigned long long ballot) {
    return __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

template <bool SCENE>
__device__ __forceinline__ void view_count_body(const ViewArgs& a) {
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    for (int k = 0; k < a.n_obj; ++k) {
        float tn, dt;
        const unsigned long long b = __ballot(view_hit(a, r, live, k, obj_samples<SCENE>(a, k), tn, dt));
        if (threadIdx.x == 0) a.blk[(long long)k * a.nb + blockIdx.x] = __popcll(b);
    }
}
__global__ void __launch_bounds__(kViewBlock) view_count(const ViewArgs a) { view_count_body<false>(a); }
__global__ void __launch_bounds__(kViewBlock) scene_view_count(const ViewArgs a) { view_count_body<true>(a); }

__global__ void __launch_bounds__(kViewScanWG) view_scan(const ViewArgs a) {
    __shared__ long long wsum[kViewScanWG / 64];
    const long long n = (long long)a.n_obj * a.nb;
    const long long carry = vscan::wg_scan_totals<kViewScanWG>(
        n, wsum, [&](long long b) { return a.blk[b]; }, [&](long long b, long long ex) { a.blk[b] = ex; });
    __syncthreads();                           // the offsets below read prefixes other lanes stored
    for (int o = threadIdx.x; o <= a.n_obj; o += kViewScanWG) a.offsets[o] = o < a.n_obj ? a.blk[(long long)o * a.nb] : carry;
}

template <bool SCENE>
__device__ __forceinline__ void view_emit_body(const ViewArgs& a) {
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    for (int k = 0; k < a.n_obj; ++k) {
        float tn, dt;
        const bool hit = view_hit(a, r, live, k, obj_samples<SCENE>(a, k), tn, dt);
        const long long at = a.blk[(long long)k * a.nb + blockIdx.x] + ballot_rank(__ballot(hit));
        if (hit && at >= 0 && at < a.cap) a.pairs[at] = vg::Pair{(int)pix, tn, dt, 0};
    }
}
__global__ void __launch_bounds__(kViewBlock) view_emit(const ViewArgs a) { view_emit_body<false>(a); }
__global__ void __launch_bounds__(kViewBlock) scene_view_emit(const ViewArgs a) { view_emit_body<true>(a); }

// one lane per object; the scene form writes the group's own object index (the field kernel of a group sees its objects alone) and
// cuts by the group's chunks per entry; entries come out in object order, so a group's entries are contiguous
template <bool SCENE>
__device__ __forceinline__ void view_plan_body(const ViewArgs& a) {
    __shared__ int wsum[kViewPlanWG / 64];
    const int k = threadIdx.x;
    const int g = obj_group<SCENE>(a, k < a.n_obj ? k : 0);
    const long long per = SCENE ? a.g_per[g] : a.plan_per;
    const int kg = SCENE && g > 0 ? k - a.g_end[g - 1] : k;
    long long chunks = 0;
    if (k < a.n_obj) chunks = ((a.offsets[k + 1] - a.offsets[k]) * obj_samples<SCENE>(a, k) + kViewChunk - 1) / kViewChunk;
    const int mine = (int)((chunks + per - 1) / per);
    int total;
    const int first = vscan::wg_exclusive_scan<kViewPlanWG>(mine, wsum, total);
    constexpr long long cap = SCENE ? vl::kScenePlanCap : vl::kViewPlanCap;
    for (int e = 0; e < mine && first + e < cap; ++e) {
        const long long c0 = e * per, c1 = c0 + per < chunks ? c0 + per : chunks;
        int* q = a.plan + 4 * (first + e);
        q[0] = kg; q[1] = (int)c0; q[2] = (int)c1; q[3] = 0;
    }
}
__global__ void __launch_bounds__(kViewPlanWG) view_plan(const ViewArgs a) { view_plan_body<false>(a); }
__global__ void __launch_bounds__(kViewPlanWG) scene_view_plan(const ViewArgs a) { view_plan_body<true>(a); }

template <bool SCENE>
__device__ __forceinline__ void view_composite_body(const ViewArgs& a) {
    __shared__ float e_tn[kViewMaxHits][kViewBlock], e_dt[kViewMaxHits][kViewBlock], e_w[kViewMaxHits][kViewBlock];
    __shared__ int e_base[kViewMaxHits][kViewBlock], e_cur[kViewMaxHits][kViewBlock], e_obj[kViewMaxHits][kViewBlock];
    __shared__ int e_S[SCENE ? kViewMaxHits : 1][kViewBlock];     // scene: the entry's own sample count
    const int lane = threadIdx.x;
    long long pix;
    vg::Ray r;
    const bool live = view_lane(a, pix, r);
    int n = 0;
    bool over = false;
    for (int k = 0; k < a.n_obj; ++k) {
        float tn, dt;
        const int g = obj_group<SCENE>(a, k);
        const int S = SCENE ? a.g_samples[g] : a.cam.samples;
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
                e_base[slot][lane] = SCENE ? (int)(at * S + a.g_shift[g]) : (int)(at * S);
                e_cur[slot][lane] = 0; e_obj[slot][lane] = k;
                if constexpr (SCENE) e_S[slot][lane] = S;
            }
        }
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
                if (e_cur[e][lane] >= (SCENE ? e_S[SCENE ? e : 0][lane] : a.cam.samples)) continue;
                const float t = vg::sample_depth(e_tn[e][lane], e_dt[e][lane], e_cur[e][lane]);
                const int o = e_obj[e][lane];
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
        const int o = e_obj[e][lane];
        if (inst < 0 || w > wbest || (w == wbest && o < inst)) { inst = o; wbest = w; }
    }
    a.depth[pix] = depth;
    a.color[3 * pix] = c0; a.color[3 * pix + 1] = c1; a.color[3 * pix + 2] = c2;
    a.opacity[pix] = opacity;
    a.instance[pix] = inst;
}
__global__ void __launch_bounds__(kViewBlock) view_composite(const ViewArgs a) { view_composite_body<false>(a); }
__global__ void __launch_bounds__(kViewBlock) scene_view_composite(const ViewArgs a) { view_composite_body<true>(a); }

}  // namespace vv
