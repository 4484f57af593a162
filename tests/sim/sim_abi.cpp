// TEST INFRASTRUCTURE: runs the kernels of vmap_amd/csrc/step_kernels.h on the CPU SIMT executor.
// Host pointers in, host pointers out.  The step's layout, plan, workspace sections, argument blocks and finalize route are the
// product's own (vmap_amd/csrc/step_plan.h, the text vmapstep.hip compiles); what a test forces on purpose is said where it enters.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <cmath>

#include "sim_launch.h"
#include "step_plan.h"

namespace {
thread_local char g_err[512] = "";
}
int vl::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int vmsim_lds_bytes() { return vk::Lds32::BYTES; }
static int g_fin_form = 0;   // step_finalize_ws: 0 = a thread per quad and row group (what small shapes get), 1 = one thread per quad (many blocks / few rows)
extern "C" void vmsim_set_finalize_form(int f) { g_fin_form = f; }
static int g_sample_split = 0;
extern "C" void vmsim_set_sample_split(int nsplit) { g_sample_split = nsplit; }   // > 1: the split form of the sampler (two launches)
// ABI v7 ray hand-off: when set, the next vmsim_step ignores `pcs` and hands the kernels origin / direction [n][R][3] + centres [n][3]
static const float* g_ray_o = nullptr; static const float* g_ray_d = nullptr; static const float* g_ray_c = nullptr;
extern "C" void vmsim_set_rays(const float* o, const float* d, const float* c) { g_ray_o = o; g_ray_d = d; g_ray_c = c; }
extern "C" void vmsim_set_schedule(int s) { sim::set_schedule(s); }   // 0 round-robin (default), 1 / 2 wave-greedy forward / reverse (sim_runtime.h)

// The plan the product makes for a shape (vl::make_plan, with or without the measurement build's forms) -> status; msg: the refusal's
// text; out: family, G, tiles, NG, NW, PR, xcd_affine of the main kernel and of the finalize, the nine section offsets, the total
extern "C" int vmsim_step_plan(const vmapstep_shape* sh, int max_steps, int measurement_build, long long out[18], char* msg, int msg_len) {
    vl::Layout L;
    vl::Plan pl;
    if (sh) vl::make_layout(sh->hidden, L);
    const int rc = vl::make_plan(sh, max_steps, measurement_build != 0, L, pl);
    std::snprintf(msg, msg_len, "%s", rc ? g_err : "");
    if (rc) return rc;
    vk::StepArgs a;
    vl::fill_step_plan(a, sh, pl, L);
    const long long v[18] = {pl.family, pl.G, pl.tiles, pl.NG, pl.NW, pl.PR, a.xcd_affine, vl::finalize_xcd_affine(a, true),
                             (long long)pl.off_ploss, (long long)pl.off_imgtab, (long long)pl.off_tab_wt, (long long)pl.off_row_tab, (long long)pl.off_pgrad,
                             (long long)pl.off_wimg, (long long)pl.off_scratch, (long long)pl.off_flags, (long long)pl.off_stats, (long long)pl.total};
    std::memcpy(out, v, sizeof(v));
    return 0;
}

// family: vl::Family.  fc[t]: [n][size_t] contiguous; grads: flat slab [n][P] in natural order (14 field tensors then B).
extern "C" int vmsim_step(int n, int R, int S, int H, int family, int G, int NW_req, int xcd_affine, int weights_bf16,
                          const float* const* fc, const float* B, const float* scale,
                          const float* pcs, const float* z, const float* gt_depth, const float* gt_rgb,
                          const uint8_t* sem, const uint8_t* dmask, float color_w, float opac_w,
                          float* grads, float* loss, float* dbg_depth, float* dbg_rgb, float* dbg_opacity,
                          float* dbg_var, int* flags, int bwd,
                          // optional fused AdamW (params updated in copies p_out [n][P], moments m, v [n][PP])
                          int do_adam, float* p_out, float* m, float* v, int step, float lr, float wd) {
    const vl::Family fam = (vl::Family)family;
    if (H % 32 != 0 || H < 32 || H > 256 || vl::hidden32(fam) != (H == 32)) return -1;
    if (G * S > vk::kMaxPts || G < 1) return -2;
    vl::Layout L;
    vl::make_layout(H, L);
    const vmapstep_tuning tun = {NW_req, VMAPSTEP_KERNEL_AUTO, 0, 0};
    const vmapstep_shape sh = {n, R, S, H, weights_bf16, 0, &tun};
    vl::Plan pl;
    pl.family = fam;
    if (vl::check_shape(&sh, 1) || vl::plan_rounds(&sh, true, pl)) return -4;
    // What the tests force, over the plan's rounds: G rays per round as they are given (also more than the object has), for
    // step_main_ws the fewest 32-point tiles that hold them, and NW_req workgroups per object (0: one per round)
    pl.G = G;
    pl.tiles = fam == vl::kWs ? (G * S <= 32 ? 1 : G * S <= 64 ? 2 : 3) : 2;
    if (G * S > vl::round_points(fam, pl.tiles) || (fam == vl::kWs && pl.tiles > (H == 256 ? 1 : H == 128 ? 3 : 2))) return -3;
    pl.NG = (R + G - 1) / G;
    pl.NW = NW_req > 0 && NW_req < pl.NG ? NW_req : pl.NG;
    if (vl::plan_sections(&sh, 1, L, pl)) return -4;

    // one workspace, every section poisoned: -1 tables and flags, 0xFF scratch, NaN floats, -7 in the row table
    std::vector<char> buf(pl.total + vl::kAlign, (char)0xFF);
    char* ws = buf.data() + (vl::kAlign - reinterpret_cast<uintptr_t>(buf.data()) % vl::kAlign) % vl::kAlign;
    auto poison = [&](size_t from, size_t to, auto value) { std::fill((decltype(value)*)(ws + from), (decltype(value)*)(ws + to), value); };
    poison(pl.off_ploss, pl.off_imgtab, (float)NAN);
    poison(pl.off_row_tab, pl.off_pgrad, -7);
    poison(pl.off_pgrad, pl.off_scratch, (float)NAN);
    poison(pl.off_stats, pl.total, (float)NAN);

    vmapstep_params params, outs, gouts;
    for (int t = 0; t < 15; ++t) {
        (t < 14 ? params.fc[t] : params.pe_B) = {const_cast<float*>(t < 14 ? fc[t] : B), L.sizes[t]};
        (t < 14 ? outs.fc[t] : outs.pe_B) = {p_out ? p_out + L.offs[t] : nullptr, L.P};
        (t < 14 ? gouts.fc[t] : gouts.pe_B) = {grads ? grads + L.offs[t] : nullptr, L.P};
    }
    const vmapstep_tensor pe_scale = {const_cast<float*>(scale), 1};
    vmapstep_batch b = {};
    b.pcs = pcs; b.pcs_stride[0] = (long long)R * S * 3; b.pcs_stride[1] = S * 3; b.pcs_stride[2] = 3; b.pcs_stride[3] = 1;
    if (g_ray_o) {
        b.pcs = nullptr;
        b.ray_o = g_ray_o; b.ray_o_stride[0] = (long long)R * 3; b.ray_o_stride[1] = 3; b.ray_o_stride[2] = 1;
        b.ray_d = g_ray_d; b.ray_d_stride[0] = (long long)R * 3; b.ray_d_stride[1] = 3; b.ray_d_stride[2] = 1;
        b.center = g_ray_c; b.center_stride = 3;
    }
    b.z = z; b.z_stride[0] = (long long)R * S; b.z_stride[1] = S; b.z_stride[2] = 1;
    b.gt_depth = gt_depth; b.gt_depth_stride[0] = R; b.gt_depth_stride[1] = 1;
    b.gt_rgb = gt_rgb; b.gt_rgb_stride[0] = R * 3; b.gt_rgb_stride[1] = 3; b.gt_rgb_stride[2] = 1;
    b.sem = sem; b.sem_stride[0] = R; b.sem_stride[1] = 1;
    b.depth_mask = dmask; b.depth_mask_stride[0] = R; b.depth_mask_stride[1] = 1;

    vk::StepArgs a;
    vl::fill_step_args(a, &sh, pl, L, &params, &pe_scale, &b, 0, color_w, opac_w, ws);
    a.prep_steps = 1; a.prep_ray_step = 0;
    if (H == 32) a.xcd_affine = xcd_affine ? 1 : 0;        // hidden 32: the block map the test asks for, whatever the workgroup count
    a.dbg_depth = dbg_depth; a.dbg_rgb = dbg_rgb; a.dbg_opacity = dbg_opacity; a.dbg_var = dbg_var;
    vk::WsArgs wa{};
    wa.s = a; wa.scratch = reinterpret_cast<char*>(a.gen_scratch); wa.tab_wt = a.tab_wt;

    if (vl::block_native_rows(fam)) sl::prep_ws(wa);
    else if (a.split) sl::prep_s32(a);
    else sl::prep_f32(a, vl::prep_f32_blocks(a, 1));
    if (fam == vl::kWp) sl::main_wp(wa, bwd);
    else if (fam == vl::kWs) sl::main_ws(wa, bwd);
    else if (a.split) sl::main_s32(a, bwd);
    else if (int rc = sl::main_f32(a, a.wide, bwd, G)) return rc;

    vk::FinalizeArgs f;
    const bool adam = do_adam && p_out;
    vl::fill_finalize_args(f, a, L, &outs, grads ? &gouts : nullptr, adam ? m : nullptr, adam ? v : nullptr, bwd != 0, loss, flags, nullptr);
    if (f.do_adam) vl::adamw_consts(f, lr, 0.9, 0.999, 1e-8f, wd, step);
    vl::FinalizeRoute route = vl::finalize_route(a, f, grads != nullptr, false);
    bool grad_pass = route == vl::kFinS32AfterGrads;
    // the tests look at the gradients AND at the table-driven update of step_finalize_h32: it gets the gradient-only pass that the
    // product launches in front of step_finalize_s32 (the product itself would take step_finalize for both)
    if (fam == vl::kH32 && f.do_adam && grads) { route = vl::kFinH32; grad_pass = true; }
    const int grid = vl::finalize_grid(f);
    if (route == vl::kFinGeneric) { sl::finalize_generic(f, grid); return 0; }
    if (grad_pass) sl::finalize_generic(vl::split_off_grad_pass(f), grid);
    vk::FinalizeHot h;
    vl::fill_hot(h, f, a, L, &outs);
    if (route == vl::kFinWs) {
        f.ws_grouped = g_fin_form == 0;          // the form the test asks for
        sl::finalize_ws(f, h, a.tab_wt);
    } else if (route == vl::kFinH32) sl::finalize_h32(f, h, grid);
    else sl::finalize_s32(f, h, grid);
    return 0;
}

// sampler: host pointers everywhere (objs is a host array of vs::SampleObject with host pointers inside)
extern "C" int vmsim_sample(const vs::SampleObject* objs, int n_obj, int W, int H, int F, int P, int n1, int n2,
                            float fx, float fy, float cx, float cy, float min_bound, float eps, float stop_eps,
                            unsigned long long seed, unsigned frame_counter,
                            const int* kf_ids, const float* u_w, const float* u_h, const float* u_z, const float* g_z,
                            float* pcs, float* z, float* gt_depth, float* gt_rgb, unsigned char* sem, unsigned char* dmask) {
    vs::SampleArgs a{};
    a.objs = objs; a.n_obj = n_obj; a.W = W; a.H = H; a.F = F; a.P = P; a.n1 = n1; a.n2 = n2;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.min_bound = min_bound; a.eps = eps; a.stop_eps = stop_eps;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32); a.frame_counter = frame_counter;
    a.rnd.kf_ids = kf_ids; a.rnd.u_w = u_w; a.rnd.u_h = u_h; a.rnd.u_z = u_z; a.rnd.g_z = g_z;
    a.pcs = pcs; a.z = z; a.gt_depth = gt_depth; a.gt_rgb = gt_rgb; a.sem = sem; a.depth_mask = dmask;
    std::vector<int> obj_max(n_obj, 0);
    if (g_sample_split > 1) { a.nsplit = g_sample_split; a.obj_max = obj_max.data(); }
    sl::sample(a, n_obj, (long long)F * P);
    return 0;
}
// the row table of step_main_ws / _wp (RowWs<NB>, wsplit_kernels.h): out[r] = flat parameter behind row element r, or -1; returns the row length
// (out == nullptr: only the length)
extern "C" int vmsim_row_table(int H, int* out) {
    if (H != 64 && H != 128 && H != 256) return -1;
    const vk::GenLayout L = vk::gen_layout(H);
    const int PR = vk::ws_row_floats(H);
    for (int r = 0; out && r < PR; ++r) {
        int t = 0, o = 0;
        const bool live = H == 256 ? vk::ws_row_source<8>(r, t, o) : H == 128 ? vk::ws_row_source<4>(r, t, o) : vk::ws_row_source<2>(r, t, o);
        out[r] = live ? L.f[t] + o : -1;
    }
    return PR;
}
extern "C" int vmsim_sample_object_size() { return (int)sizeof(vs::SampleObject); }

// query: pack the image of one object then run the query kernel of that width (host pointers)
extern "C" int vmsim_query(const float* const* fc, const float* B, const float* scale, const float* pts, long long n_pts,
                           float* occ, float* rgb, int grid, int H) {
    const vk::GenLayout GL = vk::gen_layout(H);
    std::vector<float> img(H == 32 ? vk::Img32s::BYTES / 4 : GL.imgp, NAN);
    vk::StepArgs a{};
    a.n_obj = 1; a.hidden = H; a.prep_steps = 0;
    for (int t = 0; t < 14; ++t) a.fc[t] = {const_cast<float*>(fc[t]), 0};
    a.pe_B = {const_cast<float*>(B), 0};
    a.wimg = img.data();
    vk::QueryArgs q{};
    q.wimg = img.data(); q.scale = scale; q.pts = pts; q.pts_sn = 3; q.pts_sc = 1; q.n_pts = n_pts; q.occ = occ; q.rgb = rgb;
    return sl::query(H, a, q, grid);
}
