// step_plan.h - the host logic of the fused training step, defined once: parameter layout, kernel family, rounds, workspace
// sections, and the argument blocks of the main kernel and the finalize.  Host-side inline functions only; the kernel headers are
// included for their layout constants (image sizes, LDS / scratch budgets), no kernel is instantiated here.  The C ABI unit
// (vmapstep.hip, both builds) and the CPU executor of tests/sim (sim_abi.cpp) compile this one text, so the executor lays out and
// launches what the product would; what a test forces on purpose (rays per round, workgroups per object) enters as an override of
// plan_rounds' result, in front of plan_sections.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "wide_kernels.h"
#include "wpair_kernels.h"

namespace vl {

int fail(int code, const char* fmt, ...);                                        // sets the caller's last-error text, returns code

constexpr size_t kAlign = 256;
constexpr int kMaxFrameSteps = 256;      // optimisation steps per API call (the flag array has this fixed capacity)
inline size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
constexpr const char* kMeasurementOnly = "this kernel form ships in the measurement build only (tests/tools/libvmapstep_ab.so: phase stamps and A/B forms no automatic plan launches)";

// No tuning state lives in the library: overrides of the automatic plan arrive per call in vmapstep_shape::tuning.
inline const vmapstep_tuning& tuning_of(const vmapstep_shape* sh) {
    static const vmapstep_tuning kAutoTuning = {0, VMAPSTEP_KERNEL_AUTO, 0, 0};
    return (sh && sh->tuning) ? *sh->tuning : kAutoTuning;
}

struct Layout {
    int64_t sizes[15];
    int offs[16];
    int P, PP;
};
inline void make_layout(int H, Layout& L) {
    const vk::GenLayout G = vk::gen_layout(H);
    for (int t = 0; t < 15; ++t) { L.sizes[t] = G.f[t + 1] - G.f[t]; L.offs[t] = G.f[t]; }
    L.offs[15] = G.P;
    L.P = G.P;
    L.PP = G.PP;
}

// ---- the kernel family ------------------------------------------------------------------------------------------------------------
enum Family : int {
    kH32,        // hidden 32, exact fp32: step_main_h32
    kS32,        // hidden 32 on the bf16 matrix pipe with split operands: step_main_s32 (the default at hidden 32)
    kS32Bwd6,    // ... with the six-product backward (VMAPSTEP_KERNEL_S32_BWD6)
    kGen,        // other widths, exact fp32: step_main_gen (global-memory activations, one wave per 32-point tile)
    kWide,       // hidden 128 / 256: step_main_wide<4> (one tile per workgroup, four waves per tile)
    kWs,         // hidden 64 / 128 / 256, bf16 matrix pipe: step_main_ws (one wave per output block)
    kWp,         // hidden 64 / 128, bf16 matrix pipe: step_main_wp (two waves per output block)
};
inline bool hidden32(Family f) { return f <= kS32Bwd6; }
inline bool split32(Family f) { return f == kS32 || f == kS32Bwd6; }
// step_main_ws / _wp and their finalize: rows of partial gradients in block-native order behind a row table (RowWs<NB>), a W and a
// W^T image with a table each, scratch per workgroup
inline bool block_native_rows(Family f) { return f == kWs || f == kWp; }
inline bool wt_image(Family f) { return block_native_rows(f); }
inline bool workgroup_scratch(Family f) { return block_native_rows(f) || f == kWide; }
inline bool image_table(Family f) { return hidden32(f) || block_native_rows(f); }     // flat parameter -> image position (also read by step_finalize_h32)
inline int step_args_wide(Family f) { return f == kWide ? 1 : f == kWs ? 3 : f == kWp ? 4 : 0; }   // vk::StepArgs::wide
// sample points a round of the family holds (step_main_ws: by its 32-point tiles)
static_assert(vk::ImgWs<4>::kPts == 64 && vk::ImgWs<2>::kPts == 64, "two 32-point tiles");
inline int round_points(Family f, int tiles) { return f == kWs ? 32 * tiles : f == kWp ? vk::ImgWs<4>::kPts : f == kWide ? vk::kWideTile : vk::kMaxPts; }

struct Plan {
    Family family;
    int G, NG, NW;     // rays per round, rounds per object, workgroups per object
    int tiles;         // step_main_ws: 32-point tiles per round (2; 1 = single-tile rounds when every tile gets a compute unit of its own; 3: see plan_rounds)
    int PR;            // floats per row of partial gradients: PP (flat order), or RowWs<NB>::PR (block-native rows + a row table)
    // tables: flat parameter -> image position [PP] (+ step_main_ws / _wp: -> W^T image position [PP], row element -> flat parameter [PR])
    size_t off_ploss, off_imgtab, off_tab_wt, off_row_tab, off_pgrad, off_wimg, off_scratch, off_flags, off_stats, total;
};

// what the three parts below take for granted: a shape, positive counts
inline int check_shape(const vmapstep_shape* sh, int max_steps) {
    if (!sh) return fail(VMAPSTEP_ERR_ARGUMENT, "shape is null");
    if (sh->n_obj < 1 || sh->rays < 1 || sh->samples < 1 || max_steps < 1)
        return fail(VMAPSTEP_ERR_ARGUMENT, "bad shape n=%d R=%d S=%d steps=%d", sh->n_obj, sh->rays, sh->samples, max_steps);
    return VMAPSTEP_OK;
}

// (a) The family from the shape and its tuning.  measurement_build: the library carries the A/B forms (-DVMAPSTEP_AB).
inline int plan_family(const vmapstep_shape* sh, bool measurement_build, Family& fam) {
    if (sh->hidden < 32 || sh->hidden > 256 || sh->hidden % 32 != 0)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "hidden=%d: supported widths are multiples of 32 up to 256", sh->hidden);
    if (sh->weight_dtype != VMAPSTEP_WEIGHTS_F32 && sh->weight_dtype != VMAPSTEP_WEIGHTS_BF16)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "weight_dtype=%d", sh->weight_dtype);
    if (sh->samples > vk::kMaxPts)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "samples=%d > %d", sh->samples, vk::kMaxPts);
    const vmapstep_tuning& tun = tuning_of(sh);
    const int force = tun.kernel, H = sh->hidden;
    if (force < VMAPSTEP_KERNEL_AUTO || (force > VMAPSTEP_KERNEL_WP && force != VMAPSTEP_KERNEL_S32_BWD6)) return fail(VMAPSTEP_ERR_ARGUMENT, "tuning.kernel=%d", force);
    fam = H != 32 ? kGen : force == VMAPSTEP_KERNEL_H32_F32 ? kH32 : force == VMAPSTEP_KERNEL_S32_BWD6 ? kS32Bwd6 : kS32;
    if (force == VMAPSTEP_KERNEL_S32_BWD6 && (H != 32 || sh->weight_dtype != VMAPSTEP_WEIGHTS_F32))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "VMAPSTEP_KERNEL_S32_BWD6: hidden 32 with float32 weights");
    // Wide fields (hidden 128 / 256).  step_main_wide<4>: one 32-point tile per workgroup, four waves split its output
    // blocks - for latency-bound batches where every tile gets its own workgroup (it pays the whole parameter set in
    // partial-gradient traffic per 32 points).  step_main_gen: one wave per tile.
    if (H != 32 && H % 128 == 0 && force != VMAPSTEP_KERNEL_GEN && sh->samples <= vk::kWideTile) {
        const int gw = std::min(vk::kWideTile / sh->samples, sh->rays);
        const long long tiles = (long long)sh->n_obj * ((sh->rays + gw - 1) / gw);
        if (force == VMAPSTEP_KERNEL_WIDE4 || (force == VMAPSTEP_KERNEL_AUTO && tiles <= 256)) fam = kWide;
    }
    // hidden 64 / 128: the bf16 matrix pipe with split operands (step_main_ws) unless an exact-fp32 kernel is asked for
    // step_main_ws: one wave per output block; step_main_wp: two (measured: +19 % at hidden 64, where step_main_ws leaves two of its
    // four waves without a block; within 2-3 % at hidden 128 - the automatic choice follows that)
    if ((H == 128 || H == 64) && sh->samples <= vk::ImgWs<4>::kPts) {
        if (force == VMAPSTEP_KERNEL_AUTO) fam = H == 64 ? kWp : kWs;
        else if (force == VMAPSTEP_KERNEL_WS1) fam = kWs;
        else if (force == VMAPSTEP_KERNEL_WP) fam = kWp;
    }
    // hidden 256 (the iMAP field): step_main_ws<8> - eight waves, single-tile rounds.  One round per workgroup while every round
    // gets a compute unit of its own (the 100-ray configuration: 0.232 -> 0.102 ms per step); with more rounds than compute units
    // every further round re-reads and re-writes its 1.4 MB gradient row and the step becomes bound by that traffic - still ahead
    // of the exact-fp32 kernels (the reference's own iMAP batch, 4800 rays: 3.50 -> 2.38 ms, profiles/r04i_*)
    if (H == 256 && sh->samples <= 32 && (force == VMAPSTEP_KERNEL_AUTO || force == VMAPSTEP_KERNEL_WS1)) fam = kWs;
    if (!measurement_build && split32(fam) && (tun.ws_flags & (8 | 16 | 32 | 64)))      // hidden 32, A/B forms of step_main_s32: the B_layer.weight gradient with one butterfly per value (bit 3), the former order of the global loads (bit 4), the former order of the front (bit 5), the former backward (bit 6)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "%s", kMeasurementOnly);
    if ((force == VMAPSTEP_KERNEL_WS1 || force == VMAPSTEP_KERNEL_WP) && !block_native_rows(fam))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "VMAPSTEP_KERNEL_WS1 / _WP: hidden 64 / 128 with at most 64 samples per ray (_WS1 also hidden 256 with at most 32)");
    return VMAPSTEP_OK;
}

// (b) The rounds of pl.family: rays per round, tiles per round, rounds and workgroups per object.
inline int plan_rounds(const vmapstep_shape* sh, bool measurement_build, Plan& pl) {
    const vmapstep_tuning& tun = tuning_of(sh);
    const Family fam = pl.family;
    const int cap = fam == kWs && sh->hidden == 256 ? 32 : round_points(fam, 2);      // plan_family never lets a longer ray in
    if (sh->samples > cap) return fail(VMAPSTEP_ERR_UNSUPPORTED, "samples=%d > %d", sh->samples, cap);
    pl.G = round_points(fam, 2) / sh->samples;
    pl.tiles = 2;
    if (fam == kWs) {
        // step_main_ws, tiles per round.  The kernel's time is the busiest workgroup's rounds, one workgroup per compute unit:
        //  * a mostly idle chip (the ray-sharded background model of a multi-GPU run: 150 rays per rank at 8 ranks): if every
        //    32-point tile can have a compute unit of its own, single-tile rounds (about 0.77 of a two-tile round's time) halve
        //    the points per workgroup; the extra partial-gradient rows cost the finalize ~0.1 us each (profiles/r03j_*);
        //  * more two-tile rounds than compute units (the 1200-ray background batch of ONE GPU: 300 rounds): three-tile rounds
        //    (hidden 128) if they give every workgroup exactly one round (200) - no second round, no read-modify-write of its
        //    gradient row (profiles/r03u_*).
        // tuning.ws_flags: bit 0 = never single-tile rounds, bit 1 = always three-tile rounds (hidden 128; tests), bit 2 = never
        const int g1 = 32 / sh->samples, g2 = pl.G, g3 = 96 / sh->samples;
        const bool autoplan = tun.workgroups_per_object <= 0;
        auto rounds = [&](int g) { return g >= 1 ? (long long)sh->n_obj * ((sh->rays + std::min(g, sh->rays) - 1) / std::min(g, sh->rays)) : (1LL << 40); };
        if (sh->hidden == 256) { pl.G = g1; pl.tiles = 1; }
        else if (sh->hidden == 128 && (tun.ws_flags & 2)) { pl.G = g3; pl.tiles = 3; }
        else if (autoplan && !(tun.ws_flags & 1) && rounds(g1) <= 256) { pl.G = g1; pl.tiles = 1; }
        else if (autoplan && sh->hidden == 128 && !(tun.ws_flags & 4) && rounds(g2) > 256 && rounds(g3) <= 256) { pl.G = g3; pl.tiles = 3; }
    }
    if (pl.G > sh->rays) pl.G = sh->rays;
    pl.NG = (sh->rays + pl.G - 1) / pl.G;
    // workgroup slots of the chip: one per CU, two for step_main_wp at hidden 64 (78 KB of LDS per workgroup)
    const int wg_slots = (fam == kWp && sh->hidden == 64) ? 512 : 256;
    int nw = tun.workgroups_per_object > 0 ? tun.workgroups_per_object : wg_slots / sh->n_obj;
    if (nw < 1) nw = 1;
    if (nw > pl.NG) nw = pl.NG;
    if (block_native_rows(fam) && tun.workgroups_per_object <= 0) {
        // one workgroup per CU: with more rounds than workgroup slots the busiest workgroup sets the kernel time, so spread
        // the rounds evenly (300 rounds on 256 CUs: 150 workgroups x 2 rounds) - fewer partial-gradient rows for the finalize
        const int per = (pl.NG + nw - 1) / nw;
        nw = (pl.NG + per - 1) / per;
    }
    pl.NW = nw;
    // The product library carries the kernel forms automatic plans launch (+ the exact-fp32 references step_main_h32 / _gen).  Forms
    // that exist for A/B measurements only - step_main_wide<4>, step_main_ws at hidden 64, step_main_wp at hidden 128, three-tile rounds
    // with several rounds per workgroup - and the phase-stamp instantiations live in the measurement build (tests/tools/libvmapstep_ab.so, built by __graft_entry__.build() with -DVMAPSTEP_AB).
    if (!measurement_build && (fam == kWide || (fam == kWs && sh->hidden == 64) || (fam == kWp && sh->hidden == 128) || (fam == kWs && pl.tiles == 3 && pl.NW != pl.NG)))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "%s", kMeasurementOnly);
    return VMAPSTEP_OK;
}

// (c) The workspace sections for pl's family and rounds.  The buffers that exist once per workgroup are sized for THIS plan's NW
// (the tuning is part of the shape, so the sizing call and the launches see the same plan; a mismatch is caught by the workspace
// size check of the call, never silently).  Every offset is independent of the step count (only the total grows with it): a frame
// prepared for n steps, a single prepared step of it and the optimiser-only call address the same buffers.  The per-step arrays
// come last.
// step_main_s32 fetches a step's four flags and an object's four counts as one 16-byte load each (load_obj_meta, step_kernels.h): both
// sections start on a multiple of kAlign, a step advances flags by 4 ints and stats by n_obj * 4 floats, an object by 4 floats.
static_assert(kAlign % 16 == 0 && (4 * sizeof(int)) % 16 == 0 && (4 * sizeof(float)) % 16 == 0 && alignof(vk::MetaI4) == 16 && alignof(vk::MetaF4) == 16 &&
              sizeof(vk::MetaI4) == 4 * sizeof(int) && sizeof(vk::MetaF4) == 4 * sizeof(float), "flags / stats: 16-byte vectors");
inline int plan_sections(const vmapstep_shape* sh, int max_steps, const Layout& L, Plan& pl) {
    if (max_steps > kMaxFrameSteps) return fail(VMAPSTEP_ERR_UNSUPPORTED, "steps per call %d > %d", max_steps, kMaxFrameSteps);
    const Family fam = pl.family;
    const int H = sh->hidden;
    const size_t wgs = (size_t)sh->n_obj * pl.NW, table = align_up((size_t)L.PP * sizeof(int));
    const vk::GenLayout GL = vk::gen_layout(H);
    pl.PR = block_native_rows(fam) ? vk::ws_row_floats(H) : L.PP;
    size_t image, scratch;       // bytes of one object's parameter image, of one workgroup's scratch
    if (split32(fam)) image = vk::Img32s::BYTES;
    else if (wt_image(fam)) image = H == 256 ? vk::ImgWs<8>::BYTES : H == 128 ? vk::ImgWs<4>::BYTES : vk::ImgWs<2>::BYTES;
    else image = GL.imgp * sizeof(float);
    if (fam == kWp) scratch = H == 128 ? vk::LdsWp<4>::WG_SCRATCH : vk::LdsWp<2>::WG_SCRATCH;
    else if (fam == kWs) scratch = vk::kWsScratchMax;
    else if (hidden32(fam)) scratch = 0;
    else   // register-image scratch: per wave (step_main_gen) or per workgroup (step_main_wide)
        scratch = (size_t)(workgroup_scratch(fam) ? 1 : vk::kWaves) * vk::gen_wave_blocks(GL.NB) * vk::kBlk * sizeof(float);
    size_t o = 0;
    pl.off_ploss = o; o += align_up(wgs * 4 * sizeof(float));
    pl.off_imgtab = o; o += image_table(fam) ? table : 0;
    pl.off_tab_wt = o; o += wt_image(fam) ? table : 0;
    pl.off_row_tab = o; o += block_native_rows(fam) ? align_up((size_t)pl.PR * sizeof(int)) : 0;
    pl.off_pgrad = o; o += align_up(wgs * pl.PR * sizeof(float));
    pl.off_wimg = o; o += align_up((size_t)sh->n_obj * image);
    pl.off_scratch = o; o += scratch ? align_up(wgs * scratch) : 0;
    pl.off_flags = o; o += align_up((size_t)kMaxFrameSteps * 4 * sizeof(int));
    pl.off_stats = o; o += align_up((size_t)max_steps * sh->n_obj * 4 * sizeof(float));
    pl.total = o;
    return VMAPSTEP_OK;
}

inline int make_plan(const vmapstep_shape* sh, int max_steps, bool measurement_build, const Layout& L, Plan& pl) {
    if (int rc = check_shape(sh, max_steps)) return rc;
    if (int rc = plan_family(sh, measurement_build, pl.family)) return rc;
    if (int rc = plan_rounds(sh, measurement_build, pl)) return rc;
    return plan_sections(sh, max_steps, L, pl);
}

// ---- the main kernel's arguments -------------------------------------------------------------------------------------------------
// XCD-affine block map (an object's workgroups on ONE XCD / L2), decided HERE for every kernel family - the launchers, the
// phase-profile workgroup count and fill_finalize_args read this one value:
//  * hidden 32 (step_main_s32 / _h32): only while every XCD's share still fits its 32 CUs in one round;
//  * step_main_wp (hidden 64, two workgroups per CU): from eight objects on (the grid is padded to whole groups of eight objects;
//    measured: a rank's share of configs[4] 0.2207 -> 0.2112 ms, profiles/round5q_*);
//  * step_main_ws / _gen / _wide: never (one object, or no per-object L2 reuse to keep).
inline int main_xcd_affine(Family fam, int n_obj, int NW) {
    return fam == kWp ? (n_obj >= 8 ? 1 : 0) : (hidden32(fam) && ((n_obj + 7) / 8) * NW <= 32) ? 1 : 0;
}
// workgroups of the main kernel's launch (with the affine map the grid is padded to whole groups of eight objects)
inline int main_workgroups(const vk::StepArgs& a) { return (a.xcd_affine ? 8 * ((a.n_obj + 7) / 8) : a.n_obj) * a.NW; }

// the part of StepArgs that holds no pointer: shape, plan, family
inline void fill_step_plan(vk::StepArgs& a, const vmapstep_shape* sh, const Plan& pl, const Layout& L) {
    std::memset(&a, 0, sizeof(a));
    a.n_obj = sh->n_obj; a.R = sh->rays; a.S = sh->samples;
    a.G = pl.G; a.NG = pl.NG; a.NW = pl.NW; a.PP = L.PP; a.PR = pl.PR; a.tiles = pl.tiles;
    a.xcd_affine = main_xcd_affine(pl.family, sh->n_obj, pl.NW);
    a.hidden = sh->hidden;
    a.weights_bf16 = sh->weight_dtype == VMAPSTEP_WEIGHTS_BF16 ? 1 : 0;
    a.wide = step_args_wide(pl.family);
    a.split = split32(pl.family) ? 1 : 0;
    a.bwd6 = pl.family == kS32Bwd6 ? 1 : 0;
    a.ab_flags = split32(pl.family) ? ((tuning_of(sh).ws_flags & 8) ? 1 : 0) | ((tuning_of(sh).ws_flags & 16) ? 2 : 0) | ((tuning_of(sh).ws_flags & 32) ? 4 : 0) | ((tuning_of(sh).ws_flags & 64) ? 8 : 0) : 0;
}
// the workspace sections the kernels of pl.family read and write
inline void fill_step_workspace(vk::StepArgs& a, const Plan& pl, char* ws) {
    auto ints = [&](bool have, size_t off) { return have ? reinterpret_cast<int*>(ws + off) : nullptr; };
    a.stats = reinterpret_cast<float*>(ws + pl.off_stats);
    a.flags = reinterpret_cast<int*>(ws + pl.off_flags);
    a.part_loss = reinterpret_cast<float*>(ws + pl.off_ploss);
    a.img_tab = ints(image_table(pl.family), pl.off_imgtab);
    a.tab_wt = ints(wt_image(pl.family), pl.off_tab_wt);
    a.row_tab = ints(block_native_rows(pl.family), pl.off_row_tab);
    a.part_grad = reinterpret_cast<float*>(ws + pl.off_pgrad);
    a.wimg = reinterpret_cast<float*>(ws + pl.off_wimg);
    a.gen_scratch = reinterpret_cast<float*>(ws + pl.off_scratch);
}
inline void fill_step_args(vk::StepArgs& a, const vmapstep_shape* sh, const Plan& pl, const Layout& L,
                           const vmapstep_params* params, const vmapstep_tensor* pe_scale, const vmapstep_batch* b,
                           int64_t ray0, float cw, float ow, char* ws) {
    fill_step_plan(a, sh, pl, L);
    fill_step_workspace(a, pl, ws);
    for (int t = 0; t < VMAPSTEP_NUM_FC; ++t) a.fc[t] = {params->fc[t].ptr, params->fc[t].obj_stride};
    a.pe_B = {params->pe_B.ptr, params->pe_B.obj_stride};
    a.pe_scale = {pe_scale->ptr, pe_scale->obj_stride};
    if (b->pcs) {
        a.pcs = b->pcs + ray0 * b->pcs_stride[1];
        a.pcs_so = b->pcs_stride[0]; a.pcs_sr = b->pcs_stride[1]; a.pcs_ss = b->pcs_stride[2]; a.pcs_sc = b->pcs_stride[3];
    } else {                                  // ABI v7: the rays the points are rebuilt from (load_point, step_kernels.h)
        a.ray_o = b->ray_o + ray0 * b->ray_o_stride[1];
        a.ro_so = b->ray_o_stride[0]; a.ro_sr = b->ray_o_stride[1]; a.ro_sc = b->ray_o_stride[2];
        a.ray_d = b->ray_d + ray0 * b->ray_d_stride[1];
        a.rd_so = b->ray_d_stride[0]; a.rd_sr = b->ray_d_stride[1]; a.rd_sc = b->ray_d_stride[2];
        a.center = b->center; a.ce_so = b->center_stride;
    }
    a.z = b->z + ray0 * b->z_stride[1];
    a.z_so = b->z_stride[0]; a.z_sr = b->z_stride[1]; a.z_ss = b->z_stride[2];
    a.gt_depth = b->gt_depth + ray0 * b->gt_depth_stride[1];
    a.gd_so = b->gt_depth_stride[0]; a.gd_sr = b->gt_depth_stride[1];
    a.gt_rgb = b->gt_rgb + ray0 * b->gt_rgb_stride[1];
    a.rgb_so = b->gt_rgb_stride[0]; a.rgb_sr = b->gt_rgb_stride[1]; a.rgb_sc = b->gt_rgb_stride[2];
    a.sem = b->sem + ray0 * b->sem_stride[1];
    a.sem_so = b->sem_stride[0]; a.sem_sr = b->sem_stride[1];
    a.dmask = b->depth_mask + ray0 * b->depth_mask_stride[1];
    a.dm_so = b->depth_mask_stride[0]; a.dm_sr = b->depth_mask_stride[1];
    a.color_w = cw; a.opac_w = ow;
}
// blocks of step_prep (the exact-fp32 families): one per step + the pack blocks of every object's image
inline int prep_f32_blocks(const vk::StepArgs& a, int n_steps) { return n_steps + a.n_obj * (vk::gen_layout(a.hidden).imgp / 1024); }

// ---- the finalize ----------------------------------------------------------------------------------------------------------------
// the AdamW constants of a finalize, evaluated in double and rounded once (as torch's Python-side scalars are)
inline void adamw_consts(vk::FinalizeArgs& f, double lr, double b1, double b2, float eps, double wd, int step_after) {
    f.decay = (float)(1.0 - lr * wd);
    f.one_minus_beta1 = (float)(1.0 - b1);
    f.beta2 = (float)b2;
    f.one_minus_beta2 = (float)(1.0 - b2);
    f.eps = eps;
    f.step_size = (float)(lr / (1.0 - std::pow(b1, (double)step_after)));
    f.bias_corr2_sqrt = (float)std::sqrt(1.0 - std::pow(b2, (double)step_after));
}
// the finalize's own block -> object map: hidden 32 follows the main kernel's; step_finalize_ws (hidden >= 64) deals an object's
// blocks to one XCD from eight objects on (its scattered 2-byte image stores then merge in one L2: profiles/round5p_*)
inline int finalize_xcd_affine(const vk::StepArgs& a, bool have_grad) {
    return !have_grad ? 0 : a.wide >= 3 ? (a.n_obj >= 8 ? 1 : 0) : a.xcd_affine;
}
// exp_avg, exp_avg_sq: the AdamW moments, null = no update; with them (and gradients) f.do_adam is set and adamw_consts is the caller's next call
inline void fill_finalize_args(vk::FinalizeArgs& f, const vk::StepArgs& a, const Layout& L, const vmapstep_params* params,
                               const vmapstep_params* grads, float* exp_avg, float* exp_avg_sq, bool have_grad,
                               float* loss_out, int* flags_out, float* terms_out) {
    std::memset(&f, 0, sizeof(f));
    f.n_obj = a.n_obj; f.NW = a.NW; f.PP = L.PP; f.P = L.P; f.hidden = a.hidden; f.weights_bf16 = a.weights_bf16;
    f.PR = a.PR; f.row_tab = a.row_tab;
    for (int t = 0; t < 16; ++t) f.offs[t] = L.offs[t];
    for (int t = 0; t < 15; ++t) {
        const vmapstep_tensor* pt = t < 14 ? &params->fc[t] : &params->pe_B;
        f.param[t] = {pt->ptr, pt->obj_stride};
        if (grads) {
            const vmapstep_tensor* gt = t < 14 ? &grads->fc[t] : &grads->pe_B;
            f.grad[t] = {gt->ptr, gt->obj_stride};
        }
    }
    f.part_grad = a.part_grad; f.part_loss = a.part_loss; f.wimg = a.wimg;
    f.flags_in = a.flags; f.flags_out = flags_out; f.loss_out = loss_out; f.terms_out = terms_out;
    f.color_w = a.color_w; f.opac_w = a.opac_w;
    f.have_grad = have_grad ? 1 : 0;
    f.do_adam = (exp_avg && have_grad) ? 1 : 0;
    if (f.do_adam) { f.m = exp_avg; f.v = exp_avg_sq; }
    f.xcd_affine = finalize_xcd_affine(a, have_grad);
}

// the per-quad fields of a finalize (vk::FinalizeHot) from its FinalizeArgs
inline void fill_hot(vk::FinalizeHot& h, const vk::FinalizeArgs& f, const vk::StepArgs& a, const Layout& L, const vmapstep_params* params) {
    std::memset(&h, 0, sizeof(h));
    h.m = f.m; h.v = f.v; h.part_grad = f.part_grad; h.wimg = f.wimg; h.img_tab = a.img_tab;
    h.NW = f.NW; h.PP = f.PP; h.PR = f.PR; h.weights_bf16 = f.weights_bf16;
    h.decay = f.decay; h.one_minus_beta1 = f.one_minus_beta1; h.beta2 = f.beta2; h.one_minus_beta2 = f.one_minus_beta2;
    h.eps = f.eps; h.step_size = f.step_size; h.bias_corr2_sqrt = f.bias_corr2_sqrt;
    // parameters that are views of one [n, >= P] slab in flat order (vmap_amd.driver allocates them so): one base
    // pointer instead of a per-element tensor lookup
    h.slab = params->fc[0].ptr; h.slab_stride = params->fc[0].obj_stride;
    for (int t = 1; t < 15 && h.slab; ++t) {
        const vmapstep_tensor* pt = t < 14 ? &params->fc[t] : &params->pe_B;
        if (pt->ptr != params->fc[0].ptr + L.offs[t] || pt->obj_stride != h.slab_stride) h.slab = nullptr;
    }
}

// Which finalize kernel a step gets:
//  * kFinWs: step_main_ws / _wp - one finalize for gradients to the caller and / or AdamW; the only writer of the two weight images;
//  * kFinS32: split image - the table-driven finalize is the only writer of the planes.  kFinS32AfterGrads: a caller that also wants
//    the gradients of this step gets them from a gradient-only pass of the generic kernel first (same ordered sums);
//  * kFinH32: the common training step at hidden 32 on the exact-fp32 kernel - table-driven form (same sums, same update, a third
//    of the instructions);
//  * kFinGeneric: step_finalize.
enum FinalizeRoute { kFinWs, kFinS32, kFinS32AfterGrads, kFinH32, kFinGeneric };
inline FinalizeRoute finalize_route(const vk::StepArgs& a, const vk::FinalizeArgs& f, bool grads_wanted, bool generic_finalize) {
    if (a.wide >= 3 && f.have_grad) return kFinWs;
    if (a.split && f.do_adam) return grads_wanted ? kFinS32AfterGrads : kFinS32;
    if (!generic_finalize && a.hidden == 32 && a.img_tab && f.do_adam && !grads_wanted) return kFinH32;
    return kFinGeneric;
}
// the gradient-only pass of the generic kernel in front of kFinS32AfterGrads: its arguments; the gradient outputs leave f
inline vk::FinalizeArgs split_off_grad_pass(vk::FinalizeArgs& f) {
    vk::FinalizeArgs fg = f;
    fg.do_adam = 0;
    fg.loss_out = nullptr;             // the loss / flag workgroup runs once, in the second launch
    std::memset(f.grad, 0, sizeof(f.grad));
    return fg;
}
// grid of step_finalize / _h32 / _s32.  + 1: the loss / flag reduction has a workgroup of its own (it used to ride on block 0 and
// made it the straggler)
inline int finalize_grid(const vk::FinalizeArgs& f) {
    const int bpo = (f.PP / 4 + vk::kWG - 1) / vk::kWG;
    return (!f.have_grad ? 0 : f.xcd_affine ? 8 * ((f.n_obj + 7) / 8) * bpo : f.n_obj * bpo) + 1;
}

}  // namespace vl
