// TEST INFRASTRUCTURE: runs the kernels of vmap_amd/csrc/step_kernels.h on the CPU SIMT executor.
// Host pointers in, host pointers out; mirrors the launch sequence of vmap_amd/csrc/vmapstep.hip.
#include <cstdint>
#include <cstring>
#include <vector>

#include <cmath>

#include "sim_launch.h"

namespace {
void fc_sizes(int H, int* sz) {
    const int s[14] = {H * 87, H, H * H, H, H * (H + 87), H, H * H, H, H, 1, H * (H + 42), H, 3 * H, 3};
    for (int i = 0; i < 14; ++i) sz[i] = s[i];
}
}  // namespace

extern "C" int vmsim_lds_bytes() { return vk::Lds32::BYTES; }
static int g_fin_form = 0;   // step_finalize_ws: 0 = a thread per quad and row group (what small shapes get), 1 = one thread per quad (many blocks / few rows)
extern "C" void vmsim_set_finalize_form(int f) { g_fin_form = f; }
static int g_wide = 0;
extern "C" void vmsim_set_wide(int w) { g_wide = w; }
static int g_sample_split = 0;
extern "C" void vmsim_set_sample_split(int nsplit) { g_sample_split = nsplit; }   // > 1: the split form of the sampler (two launches)
// ABI v7 ray hand-off: when set, the next vmsim_step ignores `pcs` and hands the kernels origin / direction [n][R][3] + centres [n][3]
static const float* g_ray_o = nullptr; static const float* g_ray_d = nullptr; static const float* g_ray_c = nullptr;
extern "C" void vmsim_set_rays(const float* o, const float* d, const float* c) { g_ray_o = o; g_ray_d = d; g_ray_c = c; }
extern "C" void vmsim_set_schedule(int s) { sim::set_schedule(s); }   // 0 round-robin (default), 1 / 2 wave-greedy forward / reverse (sim_runtime.h)
static int g_split = 0;
extern "C" void vmsim_set_split(int on) { g_split = on; }   // hidden 32: 1 = step_main_s32 (split-bf16 matrix pipe) instead of step_main_h32; 2 = ... with the six-product backward   

// fc[t]: [n][size_t] contiguous; grads: flat slab [n][P] in natural order (14 field tensors then B).
extern "C" int vmsim_step(int n, int R, int S, int H, int G, int NW_req, int xcd_affine, int weights_bf16,
                          const float* const* fc, const float* B, const float* scale,
                          const float* pcs, const float* z, const float* gt_depth, const float* gt_rgb,
                          const uint8_t* sem, const uint8_t* dmask, float color_w, float opac_w,
                          float* grads, float* loss, float* dbg_depth, float* dbg_rgb, float* dbg_opacity,
                          float* dbg_var, int* flags, int bwd,
                          // optional fused AdamW (params updated in copies p_out [n][P], moments m, v [n][PP])
                          int do_adam, float* p_out, float* m, float* v, int step, float lr, float wd) {
    if (H % 32 != 0 || H < 32 || H > 256) return -1;
    if (G * S > vk::kMaxPts || G < 1) return -2;
    int sz[14], offs[16];
    fc_sizes(H, sz);
    int P = 0;
    for (int t = 0; t < 14; ++t) { offs[t] = P; P += sz[t]; }
    offs[14] = P; P += 63; offs[15] = P;
    const int PP = (P + 63) / 64 * 64;
    const int NG = (R + G - 1) / G;
    const int NW = NW_req > 0 && NW_req < NG ? NW_req : NG;

    std::vector<int> fl(4, -1);
    const vk::GenLayout GL = vk::gen_layout(H);
    const bool split = g_split && H == 32;
    const bool wp = g_wide == 4 && (H == 128 || H == 64);    // step_main_wp (two waves per output block)
    const bool ws = ((g_wide == 3 || g_wide == 4) && (H == 128 || H == 64)) || (g_wide == 3 && H == 256);    // step_main_ws / _wp (split-bf16 matrix pipe, hidden 128 / 64; _ws also 256)
    const int PR = ws ? vk::ws_row_floats(H) : PP;          // floats per row of partial gradients (step_main_ws / _wp: block-native rows)
    std::vector<float> stats(n * 4, NAN), part_grad((size_t)n * NW * PR, NAN), part_loss((size_t)n * NW * 4, NAN);
    std::vector<int> row_tab(PR, -7);
    if (ws && G * S > (H == 256 ? 32 : g_wide == 3 && H == 128 ? 96 : vk::ImgWs<4>::kPts)) return -3;   // step_main_ws at hidden 128: up to three 32-point tiles per round
    std::vector<float> wimg((size_t)n * (split ? vk::Img32s::BYTES / 4 : ws ? (H == 256 ? vk::ImgWs<8>::BYTES : H == 128 ? vk::ImgWs<4>::BYTES : vk::ImgWs<2>::BYTES) / 4 : GL.imgp), NAN);

    vk::StepArgs a{};
    a.tiles = g_wide == 3 ? (G * S <= 32 ? 1 : G * S <= 64 ? 2 : 3) : 2;   // step_main_ws: the fewest 32-point tiles that hold the caller's ray groups
    a.n_obj = n; a.R = R; a.S = S; a.G = G; a.NG = NG; a.NW = NW; a.PP = PP; a.PR = PR; a.row_tab = ws ? row_tab.data() : nullptr; a.prep_steps = 1; a.prep_ray_step = 0; a.xcd_affine = (xcd_affine && H == 32) ? 1 : 0; a.hidden = H; a.weights_bf16 = weights_bf16;
    for (int t = 0; t < 14; ++t) a.fc[t] = {const_cast<float*>(fc[t]), sz[t]};
    a.pe_B = {const_cast<float*>(B), 63};
    a.pe_scale = {const_cast<float*>(scale), 1};
    a.pcs = pcs; a.pcs_so = (long long)R * S * 3; a.pcs_sr = S * 3; a.pcs_ss = 3; a.pcs_sc = 1;
    if (g_ray_o) {
        a.pcs = nullptr;
        a.ray_o = g_ray_o; a.ro_so = (long long)R * 3; a.ro_sr = 3; a.ro_sc = 1;
        a.ray_d = g_ray_d; a.rd_so = (long long)R * 3; a.rd_sr = 3; a.rd_sc = 1;
        a.center = g_ray_c; a.ce_so = 3;
    }
    a.z = z; a.z_so = (long long)R * S; a.z_sr = S; a.z_ss = 1;
    a.gt_depth = gt_depth; a.gd_so = R; a.gd_sr = 1;
    a.gt_rgb = gt_rgb; a.rgb_so = R * 3; a.rgb_sr = 3; a.rgb_sc = 1;
    a.sem = sem; a.sem_so = R; a.sem_sr = 1;
    a.dmask = dmask; a.dm_so = R; a.dm_sr = 1;
    a.color_w = color_w; a.opac_w = opac_w;
    a.stats = stats.data(); a.flags = fl.data();
    a.part_grad = part_grad.data(); a.part_loss = part_loss.data(); a.wimg = wimg.data();
    a.dbg_depth = dbg_depth; a.dbg_rgb = dbg_rgb; a.dbg_opacity = dbg_opacity; a.dbg_var = dbg_var;
    std::vector<int> img_tab(PP, -1);
    a.img_tab = H == 32 || ws ? img_tab.data() : nullptr;   // flat parameter -> image position (step_finalize_h32)
    std::vector<int> tab_wt(PP, -1);
    vk::WsArgs wa{};

    std::vector<char> ws_scratch;
    if (ws) {
        ws_scratch.assign((size_t)n * NW * (wp ? (H == 128 ? vk::LdsWp<4>::WG_SCRATCH : vk::LdsWp<2>::WG_SCRATCH) : (size_t)vk::kWsScratchMax), (char)0xFF);
        wa.s = a; wa.scratch = ws_scratch.data(); wa.tab_wt = tab_wt.data();
        sl::prep_ws(wa);
    } else if (split) sl::prep_s32(a);
    else sl::prep_f32(a, 1 + n * (vk::gen_layout(H).imgp / 1024));
    if (wp) sl::main_wp(wa, bwd);
    else if (ws) sl::main_ws(wa, bwd);
    else if (split) { a.bwd6 = (g_split == 2 && bwd && !weights_bf16) ? 1 : 0; sl::main_s32(a, bwd); }
    else if (int rc = sl::main_f32(a, g_wide, bwd, G)) return rc;

    vk::FinalizeArgs f{};
    f.n_obj = n; f.NW = NW; f.PP = PP; f.P = P; f.hidden = H; f.weights_bf16 = weights_bf16;
    f.PR = PR; f.row_tab = a.row_tab;
    for (int t = 0; t < 16; ++t) f.offs[t] = offs[t];
    for (int t = 0; t < 15; ++t) {
        f.grad[t] = {grads ? grads + offs[t] : nullptr, P};
        f.param[t] = {p_out ? p_out + offs[t] : nullptr, P};
    }
    f.m = m; f.v = v; f.wimg = wimg.data();
    f.part_grad = part_grad.data(); f.have_grad = bwd;
    f.part_loss = part_loss.data();
    f.flags_in = fl.data(); f.flags_out = flags; f.loss_out = loss;
    f.color_w = color_w; f.opac_w = opac_w;
    f.do_adam = do_adam;
    f.decay = (float)(1.0 - (double)lr * (double)wd);
    f.one_minus_beta1 = (float)(1.0 - 0.9); f.beta2 = 0.999f; f.one_minus_beta2 = (float)(1.0 - 0.999);
    f.eps = 1e-8f;
    f.step_size = (float)((double)lr / (1.0 - std::pow(0.9, step)));
    f.bias_corr2_sqrt = (float)std::sqrt(1.0 - std::pow(0.999, step));
    const int bpo = (PP / 4 + vk::kWG - 1) / vk::kWG;
    if (ws && bwd) {
        // one finalize for the gradients the tests look at and / or the AdamW update (as the library launches it)
        vk::FinalizeHot h{};
        h.m = f.m; h.v = f.v; h.part_grad = f.part_grad; h.wimg = f.wimg; h.img_tab = img_tab.data();
        h.NW = f.NW; h.PP = f.PP; h.PR = f.PR; h.weights_bf16 = f.weights_bf16;
        h.decay = f.decay; h.one_minus_beta1 = f.one_minus_beta1; h.beta2 = f.beta2; h.one_minus_beta2 = f.one_minus_beta2;
        h.eps = f.eps; h.step_size = f.step_size; h.bias_corr2_sqrt = f.bias_corr2_sqrt;
        f.do_adam = do_adam && p_out;
        f.ws_grouped = g_fin_form == 0;
        sl::finalize_ws(f, h, tab_wt.data());
        return 0;
    }
    if (H == 32 && bwd && do_adam && p_out) {
        // the table-driven form the library launches for a plain training step at hidden 32 (parameters: one [n, P] slab here);
        // the gradients the tests look at come from a gradient-only pass of the generic kernel first
        if (grads) {
            vk::FinalizeArgs fg = f;
            fg.do_adam = 0;
            sl::finalize_generic(fg, n * bpo + 1);
            for (int t = 0; t < 15; ++t) f.grad[t] = {nullptr, P};
        }
        vk::FinalizeHot h{};
        h.m = f.m; h.v = f.v; h.part_grad = f.part_grad; h.wimg = f.wimg; h.img_tab = img_tab.data();
        h.slab = p_out; h.slab_stride = P;
        h.NW = f.NW; h.PP = f.PP; h.PR = f.PR; h.weights_bf16 = f.weights_bf16;
        h.decay = f.decay; h.one_minus_beta1 = f.one_minus_beta1; h.beta2 = f.beta2; h.one_minus_beta2 = f.one_minus_beta2;
        h.eps = f.eps; h.step_size = f.step_size; h.bias_corr2_sqrt = f.bias_corr2_sqrt;
        if (split) sl::finalize_s32(f, h, n * bpo + 1);
        else sl::finalize_h32(f, h, n * bpo + 1);
        return 0;
    }
    sl::finalize_generic(f, n * bpo + 1);
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
