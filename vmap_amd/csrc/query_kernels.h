// query_kernels.h - inference query of one object field at arbitrary points.
//
// Replaces the chunked torch.no_grad() loop of the reference's Trainer.eval_points (trainer.py:77-95: pe -> fc_occ_map
// -> sigmoid, 100 000 points per chunk) that mesh extraction calls on a dense grid (render_rays.py:98-122, up to 256^3
// points per object).  Hidden 32: field_query_s32 (query_split_kernels.h: the forward of step_main_s32 on the bf16 matrix
// pipe, float32-equivalent; it replaced the exact-fp32 field_query_h32 of rounds 1-2).  Any other width 32 k <= 256:
// field_query_gen below (exact-fp32 matrix instruction, weights streamed from the object's L2-resident image).
// Persistent workgroups, each wave streams 32-point tiles; 16 B written per point against 22.3 kFLOP at hidden 32.
// field_query_seg_gen is the same forward over the segmented pair list of one field group of a view (view_kernels.h).
#pragma once
#include "step_kernels.h"
#include "launch_geometry.h"
#include "view_args.h"

namespace vk {

struct QueryArgs {
    const float* wimg;                 // packed parameter image of the object (Lds32 layout)
    const float* scale;                // pe.scale (1 float)
    const float* pts; long long pts_sn, pts_sc;    // [N,3] with element strides
    long long n_pts;
    float* occ;                        // [N]    sigmoid(alpha)   (render_rays.py:4-8 occupancy_activation)
    float* rgb;                        // [N,3]  sigmoid(raw colour)
};

// The forward of one 32-point tile at hidden width H = 32 * NB (this lane's point t = x / scale in the object frame; p31 = the
// point's column, hi = the lane's half): PE blocks, the five layers, the heads.  Wg = the object's parameter image in global
// memory (L2-resident: 0.4-1.3 MB), read 16 bytes per lane and four matrix instructions; a tile's activations stay on chip: two
// ping-pong sets of NB x 16 values per lane, both in registers up to NB = 4; from NB = 5 (where two sets no longer fit the
// 512-register file) the second set lives in the wave-private LDS area hBl in register-image form (NB x 4 KiB per wave; a lane
// only re-reads what it wrote itself).  Returns the raw alpha and colour sums, complete in both halves.  field_query_gen and
// field_query_seg_gen both call it: one body, the same bits.
template <int NB>
__device__ __forceinline__ void field_forward_gen(const float (&t)[3], int lane, int p31, int hi, const float* Wg, float* hBl,
                                                  float& ra, float& r0, float& r1, float& r2) {
    constexpr GenLayout L = gen_layout(32 * NB);
    constexpr int H = 32 * NB;
    constexpr bool LDSB = NB > 4;
    const float* Bg = Wg + L.pe_b;
    float proj[kDirs];
#pragma unroll
    for (int d = 0; d < kDirs; ++d)
        proj[d] = fmaf(t[2], Bg[3 * d + 2], fmaf(t[1], Bg[3 * d + 1], t[0] * Bg[3 * d]));
    float amax = 0.0f;
#pragma unroll
    for (int d = 0; d < kDirs; ++d) amax = fmaxf(amax, fabsf(proj[d]));
    const bool big = wv::wave_any(!(amax * (32.0f * kPi) < kSinCosFastLimit));
    float e1a[16], e1b[16], e1c[16], cf[16];
    if (__builtin_expect(!big, 1)) {
        pe_block<16, false>(e1a, cf, 0, kEmb1, 0, t, proj, hi);
        pe_block<16, false>(e1b, cf, 0, kEmb1, 1, t, proj, hi);
        pe_block<12, false>(e1c, cf, 0, kEmb1, 2, t, proj, hi);
    } else {
        pe_block<16, true>(e1a, cf, 0, kEmb1, 0, t, proj, hi);
        pe_block<16, true>(e1b, cf, 0, kEmb1, 1, t, proj, hi);
        pe_block<12, true>(e1c, cf, 0, kEmb1, 2, t, proj, hi);
    }
    float hA[NB][16], hB[LDSB ? 1 : NB][16];
    float tmp[16];
    f32x16 acc;
    // set B accessors: registers or the wave's LDS area
    auto putB = [&](int ob, const f32x16& v) {
        if constexpr (LDSB) {
            relu_to(tmp, v);
#pragma unroll
            for (int r = 0; r < 16; ++r) hBl[ob * 1024 + (r >> 2) * 256 + lane * 4 + (r & 3)] = tmp[r];   // 16-byte chunks per lane
        } else {
            relu_to(hB[ob], v);
        }
    };
    auto mmB = [&](f32x16& c, const float* w, int kb) {
        if constexpr (LDSB) {
#pragma unroll
            for (int r = 0; r < 16; ++r) tmp[r] = hBl[kb * 1024 + (r >> 2) * 256 + lane * 4 + (r & 3)];
            fwd_mm<4>(c, w, tmp);
        } else {
            fwd_mm<4>(c, w, hB[kb]);
        }
    };
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {           // in_layer -> hA
        const float* w = Wg + L.w_in + (32 * ob + p31) * L.ld_in + 4 * hi;
        load_bias(acc, Wg + L.b_in + 32 * ob, hi);
        fwd_mm<4>(acc, w, e1a); fwd_mm<4>(acc, w + 32, e1b); fwd_mm<3>(acc, w + 64, e1c);
        relu_to(hA[ob], acc);
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {           // mid1 -> hB
        const float* w = Wg + L.w_m1 + (32 * ob + p31) * L.ld_m + 4 * hi;
        load_bias(acc, Wg + L.b_m1 + 32 * ob, hi);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) fwd_mm<4>(acc, w + 32 * kb, hA[kb]);
        putB(ob, acc);
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {           // cat_layer -> hA
        const float* w = Wg + L.w_cat + (32 * ob + p31) * L.ld_cat + 4 * hi;
        load_bias(acc, Wg + L.b_cat + 32 * ob, hi);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) mmB(acc, w + 32 * kb, kb);
        fwd_mm<4>(acc, w + H, e1a); fwd_mm<4>(acc, w + H + 32, e1b); fwd_mm<3>(acc, w + H + 64, e1c);
        relu_to(hA[ob], acc);
    }
#pragma unroll
    for (int ob = 0; ob < NB; ++ob) {           // mid2 -> hB (= fc4)
        const float* w = Wg + L.w_m2 + (32 * ob + p31) * L.ld_m + 4 * hi;
        load_bias(acc, Wg + L.b_m2 + 32 * ob, hi);
#pragma unroll
        for (int kb = 0; kb < NB; ++kb) fwd_mm<4>(acc, w + 32 * kb, hA[kb]);
        putB(ob, acc);
    }
    {
        float e2a[16], e2b[16];
        if (__builtin_expect(!big, 1)) {
            pe_block<16, false>(e2a, cf, kEmb1, kEmb2, 0, t, proj, hi);
            pe_block<6, false>(e2b, cf, kEmb1, kEmb2, 1, t, proj, hi);
        } else {
            pe_block<16, true>(e2a, cf, kEmb1, kEmb2, 0, t, proj, hi);
            pe_block<6, true>(e2b, cf, kEmb1, kEmb2, 1, t, proj, hi);
        }
#pragma unroll
        for (int ob = 0; ob < NB; ++ob) {       // color_linear -> hA
            const float* w = Wg + L.w_c + (32 * ob + p31) * L.ld_c + 4 * hi;
            load_bias(acc, Wg + L.b_c + 32 * ob, hi);
#pragma unroll
            for (int kb = 0; kb < NB; ++kb) mmB(acc, w + 32 * kb, kb);
            fwd_mm<4>(acc, w + H, e2a); fwd_mm<2>(acc, w + H + 32, e2b);
            relu_to(hA[ob], acc);
        }
    }
    ra = 0.0f; r0 = 0.0f; r1 = 0.0f; r2 = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
        if constexpr (LDSB) {
#pragma unroll
            for (int r = 0; r < 16; ++r) tmp[r] = hBl[kb * 1024 + (r >> 2) * 256 + lane * 4 + (r & 3)];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = 32 * kb + phi(r, hi);
            ra = fmaf(Wg[L.w_a + j], LDSB ? tmp[r] : hB[LDSB ? 0 : kb][r], ra);
            r0 = fmaf(Wg[L.w_oc + j], hA[kb][r], r0);
            r1 = fmaf(Wg[L.w_oc + H + j], hA[kb][r], r1);
            r2 = fmaf(Wg[L.w_oc + 2 * H + j], hA[kb][r], r2);
        }
    }
    ra += wv::swap_half(ra); r0 += wv::swap_half(r0); r1 += wv::swap_half(r1); r2 += wv::swap_half(r2);
    ra += Wg[L.b_a]; r0 += Wg[L.b_oc]; r1 += Wg[L.b_oc + 1]; r2 += Wg[L.b_oc + 2];
}

// Any hidden width H = 32 * NB (NB = 2..8: the background model's 128, iMAP's 256, ...) at arbitrary points of one object.
template <int NB>
__global__ __launch_bounds__(kWG, 1) void field_query_gen(const QueryArgs a) {
    const int tid_k = threadIdx.x;
    const float* Wg = a.wimg;
    const float scale = a.scale[0];
    for (long long chunk = blockIdx.x; chunk * kMaxPts < a.n_pts; chunk += gridDim.x) {
        // lane coordinates opaque per tile: otherwise the ~5 NB^2 weight row addresses of the body are loop-invariant,
        // hoisted in front of the loop and spilled (same effect as in step_main_h32's multi-pass loop)
        const int tid = wv::opaque_iter(tid_k), lane = tid & 63, wave = tid >> 6, p31 = lane & 31, hi = lane >> 5;
        float* hBl = wv::lds_base() + wave * (NB * 1024);      // NB > 4: set B, block kb at hBl + kb * 1024, [r][lane]
        const long long pt = chunk * kMaxPts + wave * 32 + p31;
        const bool valid = pt < a.n_pts;
        float t[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
            const float* px = a.pts + pt * a.pts_sn;
            t[0] = px[0] / scale;
            t[1] = px[a.pts_sc] / scale;
            t[2] = px[2 * a.pts_sc] / scale;
        }
        float ra, r0, r1, r2;
        field_forward_gen<NB>(t, lane, p31, hi, Wg, hBl, ra, r0, r1, r2);
        if (valid && hi == 0) {
            a.occ[pt] = sigmoidf_acc(ra * 10.0f);
            a.rgb[3 * pt + 0] = sigmoidf_acc(r0);
            a.rgb[3 * pt + 1] = sigmoidf_acc(r1);
            a.rgb[3 * pt + 2] = sigmoidf_acc(r2);
        }
    }
}

// field_query_seg_gen - the same forward over the segmented pair list of one field group of a view (view_kernels.h), the wide
// counterpart of field_query_seg_s32 (query_split_kernels.h).  The argument block is the GROUP's: object k is the group's k-th
// (boxes are not read here; centers, scale, offsets and wimg start at the group's first object), cam.samples is the group's
// sample count and occ / rgb are placed so that sample s of pair pr (a global pair index) is element pr * samples + s.  Point qi
// of object k's segment is sample qi % S of pair offsets[k] + qi / S, rebuilt in registers from the 16-byte pair record, the
// camera and the object's centre (vg::pixel_ray, sample_depth, sample_point: the contract's operation order).  One plan entry
// per workgroup: one object, a run of kViewChunk-point chunks; the weights are streamed from the object's image as above.
static_assert(vv::kViewChunk == kMaxPts, "launch_geometry.h follows the chunk");
static_assert(vl::view_wide_image_floats(64) == gen_layout(64).imgp && vl::view_wide_image_floats(96) == gen_layout(96).imgp &&
              vl::view_wide_image_floats(128) == gen_layout(128).imgp && vl::view_wide_image_floats(160) == gen_layout(160).imgp &&
              vl::view_wide_image_floats(192) == gen_layout(192).imgp && vl::view_wide_image_floats(224) == gen_layout(224).imgp &&
              vl::view_wide_image_floats(256) == gen_layout(256).imgp, "launch_geometry.h follows the image");

template <int NB>
__global__ __launch_bounds__(kWG, 1) void field_query_seg_gen(const vv::ViewArgs a) {
    const int tid_k = threadIdx.x;
    const int* entry = a.plan + 4 * blockIdx.x;
    const int k = entry[0], c0 = entry[1], c1 = entry[2];
    if (k < 0 || k >= a.n_obj || c0 < 0 || c0 >= c1) return;      // not an entry the plan kernel wrote (uniform over the workgroup)
    const float scale = a.scale[k * a.scale_so];
    const float* Wg = reinterpret_cast<const float*>(a.wimg) + (long long)k * gen_layout(32 * NB).imgp;
    const long long pair0 = a.offsets[k];
    // 32-bit point indices: the samples of a call stay below 2^31 by contract, so a chunk's end fits an unsigned
    const unsigned S = (unsigned)a.cam.samples;
    const unsigned n_pts = (unsigned)((a.offsets[k + 1] - pair0) * a.cam.samples);
    const float* center = a.centers + 3 * k;
    for (int chunk = c0; chunk < c1; ++chunk) {
        const int tid = wv::opaque_iter(tid_k), lane = tid & 63, wave = tid >> 6, p31 = lane & 31, hi = lane >> 5;
        float* hBl = wv::lds_base() + wave * (NB * 1024);
        const unsigned qi = (unsigned)chunk * kMaxPts + wave * 32 + p31;
        const unsigned pi = qi / S;
        const long long pr = pair0 + pi;
        const bool valid = qi < n_pts && pr < a.cap;
        float t[3] = {0.0f, 0.0f, 0.0f};
        if (valid) {
            const vg::Pair rec = a.pairs[pr];
            const vg::Ray ray = vg::pixel_ray(a.cam, rec.pixel / a.cam.height, rec.pixel % a.cam.height);
            float x[3];
            vg::sample_point(ray, vg::sample_depth(rec.t_near, rec.dt, (int)(qi - pi * S)), center, x);
            t[0] = x[0] / scale;                               // embedding.py:83  x / self.scale
            t[1] = x[1] / scale;
            t[2] = x[2] / scale;
        }
        float ra, r0, r1, r2;
        field_forward_gen<NB>(t, lane, p31, hi, Wg, hBl, ra, r0, r1, r2);
        if (valid && hi == 0) {
            const long long pt = pair0 * a.cam.samples + qi;
            a.occ[pt] = sigmoidf_acc(ra * 10.0f);
            a.rgb[3 * pt + 0] = sigmoidf_acc(r0);
            a.rgb[3 * pt + 1] = sigmoidf_acc(r1);
            a.rgb[3 * pt + 2] = sigmoidf_acc(r2);
        }
    }
}

}  // namespace vk
