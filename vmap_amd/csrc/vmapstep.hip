// vmapstep.hip - C ABI (include/vmapstep.h) over the fused step kernels; gfx950 only.
//
// Host side of the drop-in boundary: validates shapes, lays out the caller-provided workspace, fills the
// kernel argument blocks and enqueues   step_prep -> (step_main -> step_finalize) x n_steps   on the caller's stream, each in the
// form of the plan's kernel family (step_plan.h: step_main_s32 at hidden 32, _wp at 64, _ws at 128 / 256, _gen elsewhere).
// Never allocates, never synchronises.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "launch.h"
#include "raycast_rules.h"       // brick_dim and the step limit only
// layouts only (image sizes, LDS / scratch budgets of the plan): no kernel of the headers it includes is instantiated in this unit
#include "step_plan.h"

namespace {
thread_local char g_err[512] = "";
#ifdef VMAPSTEP_AB
constexpr bool kMeasurementBuild = true;
#else
constexpr bool kMeasurementBuild = false;
#endif
}

namespace vl {
thread_local const DispatchEvents* g_dispatch_events = nullptr;
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int launched(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "%s launch: %s", what, hipGetErrorString(e));
    return VMAPSTEP_OK;
}
}  // namespace vl

namespace {
using vl::align_up;
using vl::fail;
using vl::kAlign;
using vl::Layout;
using vl::Plan;
using vl::tuning_of;

// Every entry point runs on the device that OWNS the caller's stream, whatever device is current on the calling thread (one
// process may drive several GPUs): kernel attributes, CU counts and the launches themselves are per device.  With the NULL
// stream the current device is used as it is.
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(void* stream) {
        if (!stream) return;
        int dev = -1, cur = -1;
        if (hipStreamGetDevice(static_cast<hipStream_t>(stream), &dev) != hipSuccess || hipGetDevice(&cur) != hipSuccess) { ok = false; return; }
        if (dev != cur) {
            if (hipSetDevice(dev) != hipSuccess) { ok = false; return; }
            prev = cur;
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define VMAPSTEP_ON_STREAM_DEVICE(stream)                                                                   \
    DeviceGuard device_guard_(stream);                                                                      \
    if (!device_guard_.ok) return fail(VMAPSTEP_ERR_DEVICE, "cannot switch to the device of the stream")

// Per-device facts and one-time per-device function attributes.  A process may drive several GPUs (one
// process, 8 streams): the dynamic-LDS limit of a kernel is a per-device property of the loaded code object, so "set
// once" is keyed by (device, function); lookups take a lock (a handful per API call, next to ~40 kernel launches).
constexpr int kMaxDevices = 64;
std::mutex g_dev_mutex;
int current_device() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? dev : -1;
}
}  // namespace
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel)
int vl::ensure_dynamic_lds(const void* kernel, size_t bytes, const char* what) {
    static std::vector<const void*> done[kMaxDevices];
    const int dev = current_device();
    if (dev < 0 || dev >= kMaxDevices) return fail(VMAPSTEP_ERR_DEVICE, "hipGetDevice failed");
    std::lock_guard<std::mutex> lk(g_dev_mutex);
    for (const void* k : done[dev]) if (k == kernel) return VMAPSTEP_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
    done[dev].push_back(kernel);
    return VMAPSTEP_OK;
}
namespace {

// layout and plan of a shape: all that the queries which launch nothing need
int plan_of(const vmapstep_shape* sh, int max_steps, Layout& L, Plan& pl) {
    if (!sh) return fail(VMAPSTEP_ERR_ARGUMENT, "shape is null");
    vl::make_layout(sh->hidden, L);
    return vl::make_plan(sh, max_steps, kMeasurementBuild, L, pl);
}

int check_params(const vmapstep_params* p, const char* what, bool allow_null_entries) {
    if (!p) return fail(VMAPSTEP_ERR_ARGUMENT, "%s is null", what);
    for (int t = 0; t < VMAPSTEP_NUM_FC; ++t)
        if (!p->fc[t].ptr && !allow_null_entries) return fail(VMAPSTEP_ERR_ARGUMENT, "%s.fc[%d] is null", what, t);
    if (!p->pe_B.ptr && !allow_null_entries) return fail(VMAPSTEP_ERR_ARGUMENT, "%s.pe_B is null", what);
    return VMAPSTEP_OK;
}

int check_batch(const vmapstep_batch* b) {
    if (!b) return fail(VMAPSTEP_ERR_ARGUMENT, "batch is null");
    if (!b->z || !b->gt_depth || !b->gt_rgb || !b->sem || !b->depth_mask)
        return fail(VMAPSTEP_ERR_ARGUMENT, "batch has a null tensor");
    // the sample points: either the points tensor, or (ABI v7) the rays they are rebuilt from
    if (!b->pcs && (!b->ray_o || !b->ray_d))
        return fail(VMAPSTEP_ERR_ARGUMENT, "batch has neither pcs nor (ray_o, ray_d)");
    return VMAPSTEP_OK;
}

int check_ws(void* ws, size_t bytes, const Plan& pl) {
    if (!ws) return fail(VMAPSTEP_ERR_WORKSPACE, "workspace is null");
    if (reinterpret_cast<uintptr_t>(ws) % kAlign) return fail(VMAPSTEP_ERR_WORKSPACE, "workspace not 256-byte aligned");
    if (bytes < pl.total) return fail(VMAPSTEP_ERR_WORKSPACE, "workspace %zu < required %zu bytes", bytes, pl.total);
    return VMAPSTEP_OK;
}

// The shared opening of the step entry points, in the order their checks have always had: open() - shape, device of the stream; plan() -
// layout, plan; inputs() - parameters, gradients, batch, pe_scale, outputs (each entry point says which it requires here; what it checks
// later, or not at all, it leaves out); bind() - workspace check, then the step's argument block.  An entry point's own checks go
// between them.
enum : unsigned { kGradsRequired = 1, kGradsIfGiven = 2, kScale = 4, kOutputs = 8 };
struct StepCall {
    const vmapstep_shape* sh;
    DeviceGuard dev;
    hipStream_t st;
    Layout L;
    Plan pl;
    vk::StepArgs a;
    StepCall(const vmapstep_shape* shape, void* stream) : sh(shape), dev(stream), st(static_cast<hipStream_t>(stream)) {}
    int open() const {
        if (!sh) return fail(VMAPSTEP_ERR_ARGUMENT, "shape is null");
        if (!dev.ok) return fail(VMAPSTEP_ERR_DEVICE, "cannot switch to the device of the stream");
        return VMAPSTEP_OK;
    }
    int plan(int max_steps) { return plan_of(sh, max_steps, L, pl); }
    int inputs(const vmapstep_params* params, const vmapstep_params* grads, const vmapstep_batch* batch, const vmapstep_tensor* pe_scale,
               const vmapstep_outputs* out, unsigned need) const {
        if (int rc = check_params(params, "params", false)) return rc;
        if ((need & kGradsRequired) || ((need & kGradsIfGiven) && grads))
            if (int rc = check_params(grads, "grads", true)) return rc;
        if (int rc = check_batch(batch)) return rc;
        if ((need & kScale) && (!pe_scale || !pe_scale->ptr)) return fail(VMAPSTEP_ERR_ARGUMENT, "pe_scale is null");
        if ((need & kOutputs) && (!out || !out->loss || !out->flags)) return fail(VMAPSTEP_ERR_ARGUMENT, "outputs.loss / outputs.flags are required");
        return VMAPSTEP_OK;
    }
    // the argument block of the step whose rays start at ray0 (a frame's loop fills it again per step)
    void fill(const vmapstep_params* params, const vmapstep_tensor* pe_scale, const vmapstep_batch* batch, int64_t ray0, float cw, float ow, void* ws) {
        vl::fill_step_args(a, sh, pl, L, params, pe_scale, batch, ray0, cw, ow, static_cast<char*>(ws));
    }
    int bind(const vmapstep_params* params, const vmapstep_tensor* pe_scale, const vmapstep_batch* batch, float cw, float ow, void* ws, size_t bytes) {
        if (int rc = check_ws(ws, bytes, pl)) return rc;
        fill(params, pe_scale, batch, 0, cw, ow, ws);
        a.prep_steps = 1; a.prep_ray_step = 0;
        return VMAPSTEP_OK;
    }
    void render_outputs(const vmapstep_outputs* out) { a.dbg_depth = out->render_depth; a.dbg_rgb = out->render_color; a.dbg_opacity = out->opacity; a.dbg_var = out->var; }
};

// the dominant kernel of the plan (bwd = false: the forward-only instantiation of vmapstep_render; stamps: vmapstep_profile_phases)
int launch_main(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st) {
    if (a.split) return vl::main_s32(a, bwd, stamps, st);
    if (a.wide == 4) return vl::main_wp(a, bwd, stamps, st);
    if (a.wide == 3) return vl::main_ws(a, bwd, stamps, st);
    return vl::main_f32(a, bwd, stamps, st);
}

int launch_prep(const vk::StepArgs& a, int n_steps, hipStream_t st) {
    if (a.wide >= 3) return vl::prep_ws(a, n_steps, st);
    if (a.split) return vl::prep_s32(a, n_steps, st);
    return vl::prep_f32(a, vl::prep_f32_blocks(a, n_steps), st);
}

int launch_finalize(const vk::StepArgs& a, const Layout& L, const vmapstep_params* params, const vmapstep_params* grads,
                    const vmapstep_adamw* opt, int step_after, bool have_grad, float* loss_out, int* flags_out,
                    float* terms_out, hipStream_t st, bool generic_finalize, int step_in_call = 0) {
    vk::FinalizeArgs f;
    vl::fill_finalize_args(f, a, L, params, grads, opt ? opt->exp_avg : nullptr, opt ? opt->exp_avg_sq : nullptr, have_grad, loss_out, flags_out, terms_out);
    if (f.do_adam) {
        vl::adamw_consts(f, opt->lr, opt->beta1, opt->beta2, opt->eps, opt->weight_decay, step_after);
        if (opt->bias_table) {           // device-resident step count (graph replay): the two step-dependent factors come from the table
            f.adam_tab = opt->bias_table; f.adam_cnt = opt->step_counter; f.adam_i = step_in_call; f.adam_len = opt->table_len;
        }
    }
    const int grid = vl::finalize_grid(f);
    const vl::FinalizeRoute route = vl::finalize_route(a, f, grads != nullptr, generic_finalize);
    if (route == vl::kFinGeneric) return vl::finalize_generic(f, grid, st);
    if (route == vl::kFinS32AfterGrads)
        if (int rc = vl::finalize_generic(vl::split_off_grad_pass(f), grid, st)) return rc;
    vk::FinalizeHot h;
    vl::fill_hot(h, f, a, L, params);
    if (route == vl::kFinWs) {
        f.ws_grouped = generic_finalize ? 1 : 0;
        return vl::finalize_ws(f, h, a.tab_wt, st);
    }
    return route == vl::kFinH32 ? vl::finalize_h32(f, h, grid, st) : vl::finalize_s32(f, h, grid, st);
}

}  // namespace

extern "C" {

const char* vmapstep_last_error(void) { return g_err; }
int vmapstep_abi_version(void) { return VMAPSTEP_ABI_VERSION; }

int vmapstep_param_layout(int32_t hidden, int64_t sizes[VMAPSTEP_NUM_FC + 1], int64_t* params, int64_t* padded_params) {
    if (hidden < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "hidden=%d", hidden);
    Layout L;
    vl::make_layout(hidden, L);
    if (sizes) for (int t = 0; t < 15; ++t) sizes[t] = L.sizes[t];
    if (params) *params = L.P;
    if (padded_params) *padded_params = L.PP;
    return VMAPSTEP_OK;
}

int vmapstep_workspace_bytes(const vmapstep_shape* shape, int32_t max_steps, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    Layout L;
    Plan pl;
    if (int rc = plan_of(shape, max_steps, L, pl)) return rc;
    *bytes = pl.total;
    return VMAPSTEP_OK;
}

int vmapstep_describe_plan(const vmapstep_shape* shape, int32_t max_steps, vmapstep_plan_info* info) {
    if (!info) return fail(VMAPSTEP_ERR_ARGUMENT, "info is null");
    Layout L;
    Plan pl;
    if (int rc = plan_of(shape, max_steps, L, pl)) return rc;
    std::memset(info, 0, sizeof(*info));
    const int nb = shape->hidden / 32;
    static const char* const names[] = {"step_main_h32", "step_main_s32", "step_main_s32<bwd6>", "step_main_gen", "step_main_wide<4>", "step_main_ws<%d>", "step_main_wp<%d>"};
    std::snprintf(info->kernel, sizeof(info->kernel), names[pl.family], nb);
    info->rays_per_round = pl.G;
    info->rounds_per_object = pl.NG;
    info->workgroups_per_object = pl.NW;
    info->tiles_per_round = pl.family == vl::kWs ? pl.tiles : 0;
    info->waves_per_workgroup = pl.family == vl::kWs ? (nb > 4 ? 8 : 4) : pl.family == vl::kWp ? 2 * nb : 4;
    info->single_round = pl.NG == pl.NW ? 1 : 0;
    return VMAPSTEP_OK;
}

static int fwd_bwd_impl(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                        const vmapstep_batch* batch, float color_scaling, float opacity_scaling,
                        const vmapstep_params* grads, const vmapstep_outputs* out,
                        void* workspace, size_t workspace_bytes, void* stream, bool do_prep, int step_index = 0) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open())) return rc;
    if (step_index < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "step_index=%d", step_index);
    // the workspace of a prepared frame holds at least step_index + 1 steps; no offset depends on the step count
    if ((rc = c.plan(step_index + 1))) return rc;
    if ((rc = c.inputs(params, grads, batch, pe_scale, out, kGradsRequired | kScale | kOutputs))) return rc;
    if ((rc = c.bind(params, pe_scale, batch, color_scaling, opacity_scaling, workspace, workspace_bytes))) return rc;
    vk::StepArgs& a = c.a;
    a.stats += (size_t)step_index * shape->n_obj * 4;
    a.flags += (size_t)step_index * 4;
    c.render_outputs(out);
    if (do_prep && (rc = launch_prep(a, 1, c.st))) return rc;
    if ((rc = launch_main(a, true, false, c.st))) return rc;
    return launch_finalize(a, c.L, params, grads, nullptr, 0, true, out->loss, out->flags, out->loss_terms, c.st,
                           tuning_of(shape).generic_finalize != 0);
}

int vmapstep_fwd_bwd(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                     const vmapstep_batch* batch, float color_scaling, float opacity_scaling,
                     const vmapstep_params* grads, const vmapstep_outputs* out,
                     void* workspace, size_t workspace_bytes, void* stream) {
    return fwd_bwd_impl(shape, params, pe_scale, batch, color_scaling, opacity_scaling, grads, out, workspace,
                        workspace_bytes, stream, true);
}

int vmapstep_fwd_bwd_prepared(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                              const vmapstep_batch* batch, int32_t step_index, float color_scaling, float opacity_scaling,
                              const vmapstep_params* grads, const vmapstep_outputs* out,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return fwd_bwd_impl(shape, params, pe_scale, batch, color_scaling, opacity_scaling, grads, out, workspace,
                        workspace_bytes, stream, false, step_index);
}

int vmapstep_adamw_apply(const vmapstep_shape* shape, const vmapstep_params* params, const float* grad_slab,
                         int64_t grad_stride, const vmapstep_adamw* opt, const float* loss_terms, int32_t step_index,
                         float color_scaling, float opacity_scaling, const vmapstep_outputs* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open())) return rc;
    if (step_index < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "step_index=%d", step_index);
    if ((rc = c.plan(step_index + 1))) return rc;
    const Layout& L = c.L;
    const Plan& pl = c.pl;
    if ((rc = check_params(params, "params", false))) return rc;
    if (!grad_slab || grad_stride != L.PP || reinterpret_cast<uintptr_t>(grad_slab) % 16)
        return fail(VMAPSTEP_ERR_ARGUMENT, "grad_slab: need 16-byte aligned rows of padded_params = %d floats (vmapstep_param_layout)", L.PP);
    if (!opt || !opt->exp_avg || !opt->exp_avg_sq) return fail(VMAPSTEP_ERR_ARGUMENT, "optimiser state is required");
    if (opt->bias_table) return fail(VMAPSTEP_ERR_UNSUPPORTED, "vmapstep_adamw_apply takes the step count from opt->step (bias_table must be NULL)");
    if (loss_terms && (!out || !out->loss || !out->flags)) return fail(VMAPSTEP_ERR_ARGUMENT, "loss_terms given: outputs.loss / outputs.flags are required");
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < pl.total)
        return fail(VMAPSTEP_ERR_WORKSPACE, "workspace too small / misaligned for this shape's parameter image");
    // the gradient slab plays the role of ONE row of partial gradients per object (NW = 1, row pitch = grad_stride): the
    // finalize kernels' ordered sum degenerates to a copy, their AdamW update and image rewrite are what is wanted; the
    // reduced loss terms play the role of the one row of loss partials per object
    vk::StepArgs a;
    std::memset(&a, 0, sizeof(a));
    vl::fill_step_workspace(a, pl, static_cast<char*>(workspace));           // the images and their tables (stats, scratch: not read)
    a.n_obj = shape->n_obj; a.NW = 1; a.PP = L.PP; a.hidden = shape->hidden;
    a.PR = L.PP; a.row_tab = nullptr;            // the caller's slab is in flat order
    a.weights_bf16 = shape->weight_dtype == VMAPSTEP_WEIGHTS_BF16 ? 1 : 0;
    a.split = vl::split32(pl.family) ? 1 : 0;
    a.wide = vl::step_args_wide(pl.family);
    a.xcd_affine = 0;
    a.part_grad = const_cast<float*>(grad_slab);
    a.part_loss = const_cast<float*>(loss_terms);
    a.flags += (size_t)step_index * 4;
    a.color_w = color_scaling; a.opac_w = opacity_scaling;
    return launch_finalize(a, L, params, nullptr, opt, opt->step + 1, true, loss_terms ? out->loss : nullptr,
                           loss_terms ? out->flags : nullptr, nullptr, c.st, tuning_of(shape).generic_finalize != 0);
}

int vmapstep_workspace_counts_offset(const vmapstep_shape* shape, int32_t max_steps, size_t* counts_offset) {
    if (!shape || !counts_offset) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    Layout L;
    Plan pl;
    if (int rc = plan_of(shape, max_steps, L, pl)) return rc;
    *counts_offset = pl.off_stats;
    return VMAPSTEP_OK;
}

int vmapstep_render(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                    const vmapstep_batch* batch, float color_scaling, float opacity_scaling,
                    const vmapstep_outputs* out, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open()) || (rc = c.plan(1))) return rc;
    if ((rc = c.inputs(params, nullptr, batch, pe_scale, out, kScale | kOutputs))) return rc;
    if ((rc = c.bind(params, pe_scale, batch, color_scaling, opacity_scaling, workspace, workspace_bytes))) return rc;
    c.render_outputs(out);
    if ((rc = launch_prep(c.a, 1, c.st))) return rc;
    if ((rc = launch_main(c.a, false, false, c.st))) return rc;
    return launch_finalize(c.a, c.L, params, nullptr, nullptr, 0, false, out->loss, out->flags, out->loss_terms, c.st,
                           tuning_of(shape).generic_finalize != 0);
}

static int train_steps_impl(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                            const vmapstep_batch* frame, int64_t ray_step, int32_t n_steps,
                            float color_scaling, float opacity_scaling, const vmapstep_adamw* opt,
                            const vmapstep_params* grads, const vmapstep_outputs* out,
                            void* workspace, size_t workspace_bytes, void* stream, bool do_prep, bool do_steps,
                            size_t* flags_offset, float* time_main_ms = nullptr) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open())) return rc;
    if (n_steps < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "n_steps=%d", n_steps);
    if ((rc = c.plan(n_steps))) return rc;
    if ((rc = c.inputs(params, grads, frame, pe_scale, out, kGradsIfGiven))) return rc;      // pe_scale, outputs: the steps need them, the prepare does not
    if ((rc = check_ws(workspace, workspace_bytes, c.pl))) return rc;
    if (flags_offset) *flags_offset = c.pl.off_flags;
    hipStream_t st = c.st;
    vmapstep_tensor dummy_scale = {params->fc[0].ptr, 0};
    const vmapstep_tensor* sc = pe_scale ? pe_scale : &dummy_scale;
    vk::StepArgs& a = c.a;
    const bool device_steps = do_steps && opt && opt->bias_table;
    if (device_steps && (!opt->step_counter || opt->table_len < 1)) return fail(VMAPSTEP_ERR_ARGUMENT, "bias_table given: step_counter and table_len are required");
    if (device_steps && !do_prep) return fail(VMAPSTEP_ERR_UNSUPPORTED, "the device-resident step count is advanced by vmapstep_train_steps' own first launch: not available on the prepared path");
    if (do_prep) {
        c.fill(params, sc, frame, 0, color_scaling, opacity_scaling, workspace);
        a.prep_steps = n_steps; a.prep_ray_step = ray_step;
        a.adam_counter = device_steps ? opt->step_counter : nullptr;
        if ((rc = launch_prep(a, n_steps, st))) return rc;
    }
    if (!do_steps) return VMAPSTEP_OK;
    if (!pe_scale || !pe_scale->ptr) return fail(VMAPSTEP_ERR_ARGUMENT, "pe_scale is null");
    if (!opt || !opt->exp_avg || !opt->exp_avg_sq) return fail(VMAPSTEP_ERR_ARGUMENT, "optimiser state is required");
    if (!out || !out->loss || !out->flags) return fail(VMAPSTEP_ERR_ARGUMENT, "outputs.loss / outputs.flags are required");
    // measurement only: the events live in a guard, so that every exit path (a failed launch, a failed record, a failed create
    // part-way through) destroys the ones that exist
    struct Events {
        std::vector<hipEvent_t> v;
        ~Events() { for (hipEvent_t e : v) (void)hipEventDestroy(e); }
        bool empty() const { return v.empty(); }
        hipEvent_t operator[](size_t i) const { return v[i]; }
    } ev;
    if (time_main_ms) {
        ev.v.reserve(4 * (size_t)n_steps);   // per step: stream events in front of / behind the launch, and the launch's own
                                             // dispatch begin / end events (hipExtLaunchKernel)
        for (size_t i = 0; i < 4 * (size_t)n_steps; ++i) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "hipEventCreate failed");
            ev.v.push_back(e);
        }
    }
    for (int i = 0; i < n_steps; ++i) {
        c.fill(params, pe_scale, frame, (int64_t)i * ray_step, color_scaling, opacity_scaling, workspace);
        a.stats += (size_t)i * shape->n_obj * 4;
        a.flags += (size_t)i * 4;
        const bool last = i == n_steps - 1;
        if (last) c.render_outputs(out);
        if (!ev.empty() && hipEventRecord(ev[4 * i], st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "hipEventRecord failed");
        vl::DispatchEvents de = {nullptr, nullptr};
        if (!ev.empty()) { de = {ev[4 * i + 2], ev[4 * i + 3]}; vl::g_dispatch_events = &de; }
        rc = launch_main(a, true, false, st);
        vl::g_dispatch_events = nullptr;
        if (rc) return rc;
        if (!ev.empty() && hipEventRecord(ev[4 * i + 1], st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "hipEventRecord failed");
        if ((rc = launch_finalize(a, c.L, params, last ? grads : nullptr, opt, opt->step + i + 1, true, out->loss + i, out->flags + 4 * i,
                                  last ? out->loss_terms : nullptr, st, tuning_of(shape).generic_finalize != 0, i))) return rc;
    }
    if (!ev.empty()) {                       // measurement only: the one place this library waits for the device
        bool ok = hipStreamSynchronize(st) == hipSuccess;
        double sum_dispatch = 0.0, sum_pair = 0.0;
        for (int i = 0; i < n_steps && ok; ++i) {
            float ms = 0.0f, pair = 0.0f;
            ok = hipEventElapsedTime(&ms, ev[4 * i + 2], ev[4 * i + 3]) == hipSuccess &&
                 hipEventElapsedTime(&pair, ev[4 * i], ev[4 * i + 1]) == hipSuccess;
            sum_dispatch += ms;
            sum_pair += pair;
        }
        if (!ok) return fail(VMAPSTEP_ERR_DEVICE, "event timing of the step loop failed");
        time_main_ms[0] = (float)(sum_dispatch / n_steps);             // the dispatch's own begin -> end (= a kernel trace's duration)
        time_main_ms[1] = (float)(sum_pair / n_steps);                 // stream events recorded around the launch (includes their own cost)
    }
    return VMAPSTEP_OK;
}

int vmapstep_train_steps(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                         const vmapstep_batch* frame, int64_t ray_step, int32_t n_steps,
                         float color_scaling, float opacity_scaling, const vmapstep_adamw* opt,
                         const vmapstep_params* grads, const vmapstep_outputs* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return train_steps_impl(shape, params, pe_scale, frame, ray_step, n_steps, color_scaling, opacity_scaling, opt, grads,
                            out, workspace, workspace_bytes, stream, true, true, nullptr);
}

int vmapstep_prepare(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_batch* frame,
                     int64_t ray_step, int32_t n_steps, void* workspace, size_t workspace_bytes,
                     size_t* flags_offset, void* stream) {
    if (!flags_offset) return fail(VMAPSTEP_ERR_ARGUMENT, "flags_offset is null");
    return train_steps_impl(shape, params, nullptr, frame, ray_step, n_steps, 5.0f, 10.0f, nullptr, nullptr, nullptr,
                            workspace, workspace_bytes, stream, true, false, flags_offset);
}

int vmapstep_train_steps_prepared(const vmapstep_shape* shape, const vmapstep_params* params,
                                  const vmapstep_tensor* pe_scale, const vmapstep_batch* frame, int64_t ray_step,
                                  int32_t n_steps, float color_scaling, float opacity_scaling,
                                  const vmapstep_adamw* opt, const vmapstep_params* grads,
                                  const vmapstep_outputs* out, void* workspace, size_t workspace_bytes, void* stream) {
    return train_steps_impl(shape, params, pe_scale, frame, ray_step, n_steps, color_scaling, opacity_scaling, opt, grads,
                            out, workspace, workspace_bytes, stream, false, true, nullptr);
}

int vmapstep_profile_train_steps(const vmapstep_shape* shape, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                                 const vmapstep_batch* frame, int64_t ray_step, int32_t n_steps,
                                 float color_scaling, float opacity_scaling, const vmapstep_adamw* opt,
                                 const vmapstep_outputs* out, void* workspace, size_t workspace_bytes, void* stream,
                                 float main_kernel_ms[2]) {
    if (!main_kernel_ms) return fail(VMAPSTEP_ERR_ARGUMENT, "main_kernel_ms is null");
    return train_steps_impl(shape, params, pe_scale, frame, ray_step, n_steps, color_scaling, opacity_scaling, opt,
                            nullptr, out, workspace, workspace_bytes, stream, true, true, nullptr, main_kernel_ms);
}

int vmapstep_profile_main_kernel(const vmapstep_shape* shape, const vmapstep_params* params,
                                 const vmapstep_tensor* pe_scale, const vmapstep_batch* batch, int32_t reps,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open()) || (rc = c.plan(1))) return rc;
    if ((rc = c.inputs(params, nullptr, batch, pe_scale, nullptr, kScale))) return rc;
    if ((rc = c.bind(params, pe_scale, batch, 5.0f, 10.0f, workspace, workspace_bytes))) return rc;
    if ((rc = launch_prep(c.a, 1, c.st))) return rc;
    for (int i = 0; i < reps; ++i)
        if ((rc = launch_main(c.a, true, false, c.st))) return rc;
    return VMAPSTEP_OK;
}

int vmapstep_profile_phases(const vmapstep_shape* shape, const vmapstep_params* params,
                            const vmapstep_tensor* pe_scale, const vmapstep_batch* batch,
                            uint32_t* timing, size_t timing_elems, int32_t* n_workgroups,
                            void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    StepCall c(shape, stream);
    if ((rc = c.open()) || (rc = c.plan(1))) return rc;
    if ((rc = c.inputs(params, nullptr, batch, pe_scale, nullptr, kScale))) return rc;
    if (!timing || !n_workgroups) return fail(VMAPSTEP_ERR_ARGUMENT, "timing / n_workgroups is null");
    if (!vl::hidden32(c.pl.family) && (!vl::block_native_rows(c.pl.family) || shape->hidden == 256))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "phase stamps exist in the hidden=32 kernels and step_main_ws / _wp at hidden 64 / 128 only");
    const size_t need = (size_t)8 * ((shape->n_obj + 7) / 8) * c.pl.NW * vk::kWaves * vk::kMarks;
    if (timing_elems < need) return fail(VMAPSTEP_ERR_ARGUMENT, "timing buffer %zu < %zu elements", timing_elems, need);
    if ((rc = c.bind(params, pe_scale, batch, 5.0f, 10.0f, workspace, workspace_bytes))) return rc;
    c.a.timing = timing;
    *n_workgroups = vl::main_workgroups(c.a);
    if ((rc = launch_prep(c.a, 1, c.st))) return rc;
    return launch_main(c.a, true, true, c.st);   // the stamped instantiation
}

int vmapstep_query_workspace_bytes(int32_t hidden, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (hidden < 32 || hidden > 256 || hidden % 32 != 0)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "hidden=%d: supported widths are multiples of 32 up to 256", hidden);
    // hidden 32: the split image of field_query_s32 (80 KiB); other widths: the float32 image of field_query_gen
    *bytes = hidden == 32 ? align_up((size_t)vk::Img32s::BYTES) : align_up((size_t)vk::gen_layout(hidden).imgp * sizeof(float));
    return VMAPSTEP_OK;
}

int vmapstep_query_points(int32_t hidden, const vmapstep_params* params, const vmapstep_tensor* pe_scale, int32_t obj_index,
                          const float* points, int64_t n_points, const int64_t points_stride[2],
                          float* occupancy, float* color, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    size_t need = 0;
    if ((rc = vmapstep_query_workspace_bytes(hidden, &need))) return rc;
    if ((rc = check_params(params, "params", false))) return rc;
    if (!pe_scale || !pe_scale->ptr || !points || !points_stride || !occupancy || !color || obj_index < 0 || n_points < 0)
        return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "workspace must be 256-byte aligned and >= %zu bytes", need);
    if (n_points == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    // pack this object's image (step_prep's pack role, zero mask-statistics blocks), then the query kernel
    vk::StepArgs a;
    std::memset(&a, 0, sizeof(a));
    a.n_obj = 1; a.hidden = hidden; a.prep_steps = 0;
    for (int t = 0; t < VMAPSTEP_NUM_FC; ++t) a.fc[t] = {params->fc[t].ptr + (long long)obj_index * params->fc[t].obj_stride, 0};
    a.pe_B = {params->pe_B.ptr + (long long)obj_index * params->pe_B.obj_stride, 0};
    a.wimg = static_cast<float*>(workspace);
    vk::QueryArgs q;
    q.wimg = a.wimg;
    q.scale = pe_scale->ptr + (long long)obj_index * pe_scale->obj_stride;
    q.pts = points; q.pts_sn = points_stride[0]; q.pts_sc = points_stride[1];
    q.n_pts = n_points; q.occ = occupancy; q.rgb = color;
    return vl::query_points(hidden, a, q, n_points, static_cast<hipStream_t>(stream));
}

static int check_mesh_shape(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > 1024 || ny > 1024 || nz > 1024 || 3 * (long long)nx * ny * nz >= (1ll << 31))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "mesh volume %dx%dx%d: each side 2..1024 and 3*nx*ny*nz < 2^31", nx, ny, nz);
    return VMAPSTEP_OK;
}

static int check_mesh_workspace(int32_t nx, int32_t ny, int32_t nz, void* workspace, size_t workspace_bytes) {
    const size_t need = vl::mesh_layout(nx, ny, nz).bytes;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "mesh workspace must be 256-byte aligned and >= %zu bytes", need);
    return VMAPSTEP_OK;
}

int vmapstep_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    *bytes = vl::mesh_layout(nx, ny, nz).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_mesh_grid_points(int32_t nx, int32_t ny, int32_t nz, const float affine[12], float* points, void* stream) {
    if (!affine || !points) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::mesh_grid_points(nx, ny, nz, affine, points, static_cast<hipStream_t>(stream));
}

int vmapstep_mesh_count_valid(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream) {
    if (!volume || !counts) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    if (int rc = check_mesh_workspace(nx, ny, nz, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::mesh_count(volume, valid, nx, ny, nz, level, reinterpret_cast<long long*>(counts), workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_mesh_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream) {
    return vmapstep_mesh_count_valid(volume, nullptr, nx, ny, nz, level, counts, workspace, workspace_bytes, stream);
}

int vmapstep_mesh_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float level, const float affine[12],
                       float* vertices, float* normals, int32_t* faces, int64_t n_vertices, int64_t n_faces,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return vmapstep_mesh_emit_valid(volume, nullptr, nx, ny, nz, level, affine, vertices, normals, faces, nullptr, n_vertices, n_faces,
                                    workspace, workspace_bytes, stream);
}

int vmapstep_mesh_emit_valid(const float* volume, const uint8_t* valid, int32_t nx, int32_t ny, int32_t nz, float level,
                             const float affine[12], float* vertices, float* normals, int32_t* faces, int32_t* edge_ids,
                             int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes, void* stream) {
    if (!volume || n_vertices < 0 || n_faces < 0 || (n_vertices > 0 && !vertices) || (n_faces > 0 && !faces))
        return fail(VMAPSTEP_ERR_ARGUMENT, "null argument / negative count");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    if (int rc = check_mesh_workspace(nx, ny, nz, workspace, workspace_bytes)) return rc;
    float ninv[9];
    if (affine) {
        // the normals' map: the inverse transpose of the linear part, in double
        double m[9], inv[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[3 * r + c] = affine[4 * r + c];
        inv[0] = m[4] * m[8] - m[5] * m[7]; inv[1] = m[2] * m[7] - m[1] * m[8]; inv[2] = m[1] * m[5] - m[2] * m[4];
        inv[3] = m[5] * m[6] - m[3] * m[8]; inv[4] = m[0] * m[8] - m[2] * m[6]; inv[5] = m[2] * m[3] - m[0] * m[5];
        inv[6] = m[3] * m[7] - m[4] * m[6]; inv[7] = m[1] * m[6] - m[0] * m[7]; inv[8] = m[0] * m[4] - m[1] * m[3];
        const double det = m[0] * inv[0] + m[1] * inv[3] + m[2] * inv[6];
        if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return fail(VMAPSTEP_ERR_ARGUMENT, "mesh affine: singular linear part");
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) ninv[3 * r + c] = (float)(inv[3 * c + r] / det);     // (A^-1)^T
    }
    if (n_vertices == 0 && n_faces == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::mesh_emit(volume, valid, nx, ny, nz, level, affine, affine ? ninv : nullptr, vertices, normals, faces, edge_ids, n_vertices, n_faces,
                         workspace, static_cast<hipStream_t>(stream));
}

static int check_eval_workspace(void* workspace, size_t workspace_bytes, size_t need, const char* what) {
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "%s workspace must be 256-byte aligned and >= %zu bytes", what, need);
    return VMAPSTEP_OK;
}

// the host copy of a CSR offset array over an array of n elements: non-decreasing, inside [0, n], n < 2^31
static int check_offsets(const int64_t* off, int32_t n_sets, int64_t n, const char* what) {
    if (!off) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: host offsets are null", what);
    if (n < 0 || n >= (1ll << 31)) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: %lld points (0 .. 2^31 - 1 per array)", what, (long long)n);
    if (off[0] < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: offsets start below 0", what);
    for (int32_t s = 0; s < n_sets; ++s)
        if (off[s + 1] < off[s]) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: offsets decrease at set %d", what, (int)s);
    if (off[n_sets] > n) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: offsets run past the array (%lld > %lld)", what, (long long)off[n_sets], (long long)n);
    return VMAPSTEP_OK;
}

int vmapstep_nn_workspace_bytes(int64_t n_queries, int32_t n_sets, size_t* bytes) {
    if (!bytes || n_queries < 0 || n_queries >= (1ll << 31) || n_sets < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    *bytes = vl::nn_layout(n_queries, n_sets).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_nn_distance(const float* queries, int64_t n_queries, const int64_t* query_offsets, const int64_t* query_offsets_host,
                         const float* refs, int64_t n_refs, const int64_t* ref_offsets, const int64_t* ref_offsets_host, int32_t n_sets,
                         float* dist, int32_t* index, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_sets < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "n_sets must be >= 1");
    if (int rc = check_offsets(query_offsets_host, n_sets, n_queries, "nn queries")) return rc;
    if (int rc = check_offsets(ref_offsets_host, n_sets, n_refs, "nn refs")) return rc;
    const int64_t* qo = query_offsets_host;
    const int64_t* ro = ref_offsets_host;
    for (int32_t s = 0; s < n_sets; ++s)
        if (qo[s + 1] > qo[s] && ro[s + 1] == ro[s]) return fail(VMAPSTEP_ERR_ARGUMENT, "nn set %d has queries and no refs", (int)s);
    if (qo[n_sets] == qo[0]) return VMAPSTEP_OK;           // no query anywhere: nothing to write
    if (!queries || !refs || !query_offsets || !ref_offsets || !dist) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::nn_layout(n_queries, n_sets).bytes, "nn")) return rc;
    const vl::NnPlan plan = vl::nn_plan_host(reinterpret_cast<const long long*>(qo), reinterpret_cast<const long long*>(ro), n_sets, n_queries);
    if (plan.items >= (1ll << 31)) return fail(VMAPSTEP_ERR_UNSUPPORTED, "nn: %lld work items", (long long)plan.items);
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::nn_distance(plan, queries, reinterpret_cast<const long long*>(query_offsets), refs, reinterpret_cast<const long long*>(ref_offsets),
                           n_sets, dist, index, workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_surface_sample_workspace_bytes(int64_t n_faces, size_t* bytes) {
    if (!bytes || n_faces < 0 || n_faces >= (1ll << 31)) return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    *bytes = vl::surface_sample_bytes(n_faces);
    return VMAPSTEP_OK;
}

int vmapstep_surface_sample(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                            const int64_t* face_offsets, const int64_t* face_offsets_host, const int64_t* out_offsets,
                            const int64_t* out_offsets_host, int32_t n_sets, uint64_t seed, uint32_t stream_id, int32_t set_base,
                            const vmapstep_surface_randoms* randoms, float* points, int32_t* face_index,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (n_sets < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "n_sets must be >= 1");
    if (n_vertices < 0 || n_vertices >= (1ll << 31)) return fail(VMAPSTEP_ERR_ARGUMENT, "surface sample: %lld vertices", (long long)n_vertices);
    if (int rc = check_offsets(face_offsets_host, n_sets, n_faces, "surface sample faces")) return rc;
    if (int rc = check_offsets(out_offsets_host, n_sets, (1ll << 31) - 1, "surface sample points")) return rc;
    const int64_t* fo = face_offsets_host;
    const int64_t* oo = out_offsets_host;
    for (int32_t s = 0; s < n_sets; ++s)
        if (oo[s + 1] > oo[s] && fo[s + 1] == fo[s]) return fail(VMAPSTEP_ERR_ARGUMENT, "surface sample set %d has points and no faces", (int)s);
    if (randoms && (!randoms->u0 || !randoms->r)) return fail(VMAPSTEP_ERR_ARGUMENT, "surface sample randoms: u0 and r are both required");
    if (oo[n_sets] == oo[0]) return VMAPSTEP_OK;
    if (!vertices || !faces || !face_offsets || !out_offsets || !points) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::surface_sample_bytes(n_faces), "surface sample")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::surface_sample(vertices, n_vertices, faces, reinterpret_cast<const long long*>(face_offsets),
                              reinterpret_cast<const long long*>(out_offsets), n_sets, oo[0], oo[n_sets], seed, stream_id, set_base,
                              randoms ? randoms->u0 : nullptr, randoms ? randoms->r : nullptr, points, face_index, workspace,
                              static_cast<hipStream_t>(stream));
}

static int check_clip(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float box[15]) {
    if (n_vertices < 0 || n_vertices >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "clip box: counts 0 .. 2^31 - 1");
    if (!box || (n_faces > 0 && (!vertices || !faces))) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    for (int i = 0; i < 15; ++i)
        if (!std::isfinite(box[i])) return fail(VMAPSTEP_ERR_ARGUMENT, "clip box: non-finite box");
    return VMAPSTEP_OK;
}

int vmapstep_clip_box_workspace_bytes(int64_t n_faces, size_t* bytes) {
    if (!bytes || n_faces < 0 || n_faces >= (1ll << 31)) return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    *bytes = vl::clip_box_bytes(n_faces);
    return VMAPSTEP_OK;
}

int vmapstep_clip_box_count(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float box[15],
                            int64_t* count, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_clip(vertices, n_vertices, faces, n_faces, box)) return rc;
    if (!count) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::clip_box_bytes(n_faces), "clip box")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::clip_box_count(vertices, n_vertices, faces, n_faces, box, reinterpret_cast<long long*>(count), workspace,
                              static_cast<hipStream_t>(stream));
}

int vmapstep_clip_box_emit(const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces, const float box[15],
                           float* triangles, int64_t n_triangles, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_clip(vertices, n_vertices, faces, n_faces, box)) return rc;
    if (n_triangles < 0 || (n_triangles > 0 && !triangles)) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument / negative count");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::clip_box_bytes(n_faces), "clip box")) return rc;
    if (n_triangles == 0 || n_faces == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::clip_box_emit(vertices, n_vertices, faces, n_faces, box, triangles, n_triangles, workspace, static_cast<hipStream_t>(stream));
}

static int check_unproject(const float* depth, const int32_t* inst, const float* t_wc, int32_t n_slots, int32_t width, int32_t height,
                           const float intrinsics[4], const int32_t* pairs, const int32_t* first_pair, const int32_t* first_pair_host,
                           int32_t n_obj, int32_t n_pairs) {
    if (n_slots < 1 || width < 1 || height < 1 || width > 16384 || height > 16384 || n_obj < 1 || n_obj > 65535 || n_pairs < 0 || n_pairs > 65535)
        return fail(VMAPSTEP_ERR_ARGUMENT, "unproject: n_slots=%d width=%d height=%d n_obj=%d n_pairs=%d", n_slots, width, height, n_obj, n_pairs);
    if (!depth || !inst || !t_wc || !intrinsics || !first_pair || !first_pair_host || (n_pairs > 0 && !pairs))
        return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (!std::isfinite(intrinsics[0]) || !std::isfinite(intrinsics[1]) || !std::isfinite(intrinsics[2]) || !std::isfinite(intrinsics[3]) ||
        intrinsics[0] == 0.0f || intrinsics[1] == 0.0f)
        return fail(VMAPSTEP_ERR_ARGUMENT, "unproject: intrinsics must be finite with fx, fy != 0");
    if (first_pair_host[0] != 0 || first_pair_host[n_obj] != n_pairs) return fail(VMAPSTEP_ERR_ARGUMENT, "unproject: first_pair must run from 0 to n_pairs");
    for (int32_t o = 0; o < n_obj; ++o)
        if (first_pair_host[o + 1] < first_pair_host[o]) return fail(VMAPSTEP_ERR_ARGUMENT, "unproject: first_pair decreases at object %d", (int)o);
    return VMAPSTEP_OK;
}

static vl::UnprojectFrames unproject_frames(const float* depth, const int32_t* inst, const float* t_wc, int32_t n_slots, int32_t width,
                                            int32_t height, const float k[4]) {
    return vl::UnprojectFrames{depth, inst, t_wc, n_slots, width, height, k[0], k[1], k[2], k[3]};
}

int vmapstep_unproject_workspace_bytes(int32_t n_pairs, int32_t n_obj, int32_t width, int32_t height, size_t* bytes) {
    if (!bytes || n_pairs < 0 || n_pairs > 65535 || n_obj < 1 || n_obj > 65535 || width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    *bytes = vl::unproject_layout(n_pairs, n_obj, width, height).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_unproject_count(const float* depth, const int32_t* inst, const float* t_wc, int32_t n_slots, int32_t width, int32_t height,
                             const float intrinsics[4], const int32_t* pairs, const int32_t* first_pair, const int32_t* first_pair_host,
                             int32_t n_obj, int32_t n_pairs, int64_t* offsets, float* bounds,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_unproject(depth, inst, t_wc, n_slots, width, height, intrinsics, pairs, first_pair, first_pair_host, n_obj, n_pairs)) return rc;
    if (!offsets || !bounds) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::unproject_layout(n_pairs, n_obj, width, height).bytes, "unproject")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::unproject_count(unproject_frames(depth, inst, t_wc, n_slots, width, height, intrinsics), pairs, first_pair, n_obj, n_pairs,
                               reinterpret_cast<long long*>(offsets), bounds, workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_unproject_emit(const float* depth, const int32_t* inst, const float* t_wc, int32_t n_slots, int32_t width, int32_t height,
                            const float intrinsics[4], const int32_t* pairs, const int32_t* first_pair, const int32_t* first_pair_host,
                            int32_t n_obj, int32_t n_pairs, float* points, int64_t n_points,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_unproject(depth, inst, t_wc, n_slots, width, height, intrinsics, pairs, first_pair, first_pair_host, n_obj, n_pairs)) return rc;
    if (n_points < 0 || n_points >= (1ll << 31) || (n_points > 0 && !points)) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument / bad count");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::unproject_layout(n_pairs, n_obj, width, height).bytes, "unproject")) return rc;
    if (n_points == 0 || n_pairs == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::unproject_emit(unproject_frames(depth, inst, t_wc, n_slots, width, height, intrinsics), pairs, first_pair, n_obj, n_pairs,
                              points, n_points, workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_obb_extents(const float* points, int64_t n_points, const int64_t* offsets, const int64_t* offsets_host, int32_t n_obj,
                         const float* center, const float* rotations, int64_t set_stride, int32_t K, int32_t point_chunks,
                         float* lo, float* hi, void* stream) {
    if (n_obj < 1 || n_obj > 65535) return fail(VMAPSTEP_ERR_ARGUMENT, "obb extents: n_obj=%d (1 .. 65535)", n_obj);
    if (K < 1 || (int64_t)n_obj * K * 3 >= (1ll << 31)) return fail(VMAPSTEP_ERR_ARGUMENT, "obb extents: K=%d (K >= 1, n_obj * K * 3 < 2^31)", K);
    if (set_stride != 0 && set_stride < 9ll * K) return fail(VMAPSTEP_ERR_ARGUMENT, "obb extents: set_stride=%lld (0 or >= 9 K)", (long long)set_stride);
    if (point_chunks < 0 || point_chunks > 65535) return fail(VMAPSTEP_ERR_ARGUMENT, "obb extents: point_chunks=%d (0 .. 65535)", point_chunks);
    if (int rc = check_offsets(offsets_host, n_obj, n_points, "obb extents")) return rc;
    if (!offsets || !rotations || !lo || !hi || (n_points > 0 && !points)) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    const long long* po = reinterpret_cast<const long long*>(offsets_host);
    const int chunks = point_chunks > 0 ? point_chunks : vl::obb_chunks(po, n_obj, K);
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::obb_extents(points, reinterpret_cast<const long long*>(offsets), n_obj, center, rotations, set_stride, K, chunks, lo, hi,
                           static_cast<hipStream_t>(stream));
}

int vmapstep_cloud_moments(const float* points, int64_t n_points, const int64_t* offsets, const int64_t* offsets_host, int32_t n_obj,
                           const float* center, double* moments, void* stream) {
    if (n_obj < 1 || n_obj > 65535) return fail(VMAPSTEP_ERR_ARGUMENT, "cloud moments: n_obj=%d (1 .. 65535)", n_obj);
    if (int rc = check_offsets(offsets_host, n_obj, n_points, "cloud moments")) return rc;
    if (!offsets || !moments || (n_points > 0 && !points)) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::cloud_moments(points, reinterpret_cast<const long long*>(offsets), n_obj, center, moments, static_cast<hipStream_t>(stream));
}

static_assert(sizeof(vmapstep_sample_object) == sizeof(vs::SampleObject), "sample object table layout");

// ---- view rendering ----------------------------------------------------------------------------------------------------------------
// ONE implementation: field groups of their own hidden width and sample count composited into one image.  vmapstep_scene_view_* are
// its entry points; vmapstep_view_* are the one-group hidden-32 case of them: after their own argument checks (their limits, messages
// and order are the ABI's) they fill one vmapstep_view_group from the cfg and call the same bodies.
static_assert(VMAPSTEP_VIEW_MAX_GROUPS == vv::kViewMaxGroups, "one group limit");
constexpr int kViewFrontPlanCap = vl::kViewWgTarget + vv::kViewMaxObj;      // the 768 plan entries vmapstep_view_workspace_bytes documents

// what an entry point hands to the shared bodies, after its own limits
struct ViewCall {
    const char* name;                          // the prefix of every message: "view" | "scene view"
    const vmapstep_view_cfg* cfg;
    const vmapstep_view_group* groups;
    int n_groups, plan_cap;
};

static int check_camera(const char* name, const vmapstep_view_cfg* c) {
    if (c->pix_begin < 0 || c->pix_end < c->pix_begin || c->pix_end > (int64_t)c->width * c->height)
        return fail(VMAPSTEP_ERR_ARGUMENT, "%s: pixel range [%lld, %lld) outside the image", name, (long long)c->pix_begin, (long long)c->pix_end);
    if (!(std::isfinite(c->fx) && std::isfinite(c->fy) && std::isfinite(c->cx) && std::isfinite(c->cy)) || c->fx == 0.0f || c->fy == 0.0f)
        return fail(VMAPSTEP_ERR_ARGUMENT, "%s: intrinsics must be finite with fx, fy != 0", name);
    return VMAPSTEP_OK;
}

static vl::SceneLayout view_layout_of(const ViewCall& v, vl::SceneGroup* g) {
    for (int i = 0; i < v.n_groups; ++i) g[i] = vl::SceneGroup{v.groups[i].hidden, v.groups[i].n_obj, v.groups[i].samples};
    return vl::scene_layout(g, v.n_groups, v.cfg->pix_begin, v.cfg->pix_end, v.plan_cap);
}

static int check_view_workspace(const ViewCall& v, const vl::SceneLayout& l, void* workspace, size_t workspace_bytes) {
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < l.bytes)
        return fail(VMAPSTEP_ERR_WORKSPACE, "%s workspace must be 256-byte aligned and >= %zu bytes", v.name, l.bytes);
    return VMAPSTEP_OK;
}

static vv::ViewArgs view_args(const ViewCall& v, const vl::SceneGroup* g, const vl::SceneLayout& l, const float* boxes, void* workspace) {
    const vmapstep_view_cfg* c = v.cfg;
    vv::ViewArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam.fx = c->fx; a.cam.fy = c->fy; a.cam.cx = c->cx; a.cam.cy = c->cy;
    std::memcpy(a.cam.T, c->t_wc, sizeof(a.cam.T));
    a.cam.min_depth = c->min_depth; a.cam.width = c->width; a.cam.height = c->height;
    a.cam.samples = v.n_groups == 1 ? g[0].samples : 0;                    // view_composite<false>; the field launches set their own
    a.n_obj = l.n_obj; a.pix_begin = c->pix_begin; a.pix_end = c->pix_end; a.nb = vl::view_blocks(c->pix_begin, c->pix_end);
    a.boxes = boxes;
    char* ws = static_cast<char*>(workspace);
    a.wimg = ws;
    a.blk = reinterpret_cast<long long*>(ws + l.off_blk);
    a.plan = reinterpret_cast<int*>(ws + l.off_plan);
    a.plan_cap = l.plan_cap;
    int end = 0;
    for (int i = 0; i < vv::kViewMaxGroups; ++i) {
        if (i < v.n_groups) end += g[i].n_obj;
        a.g_end[i] = end;
        a.g_samples[i] = i < v.n_groups ? g[i].samples : 1;
        a.g_per[i] = 1;
    }
    return a;
}

static int view_count_body(const ViewCall& v, const float* boxes, int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
    if (!boxes || !offsets) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: null argument", v.name);
    vl::SceneGroup g[vv::kViewMaxGroups];
    const vl::SceneLayout l = view_layout_of(v, g);
    if (int rc = check_view_workspace(v, l, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    vv::ViewArgs a = view_args(v, g, l, boxes, workspace);
    a.offsets = reinterpret_cast<long long*>(offsets);
    return vl::view_count(a, static_cast<hipStream_t>(stream));
}

static int view_render_body(const ViewCall& v, const float* boxes, const float* centers, const int64_t* offsets, const int64_t* offsets_host,
                            void* pairs, int64_t n_pairs, float* sample_occ, float* sample_rgb,
                            float* depth, float* color, float* opacity, int32_t* instance, int32_t* overflow,
                            void* workspace, size_t workspace_bytes, void* stream) {
    vl::SceneGroup g[vv::kViewMaxGroups];
    const vl::SceneLayout l = view_layout_of(v, g);
    const int n_obj = l.n_obj;
    if (n_pairs < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: n_pairs=%lld", v.name, (long long)n_pairs);
    if (!offsets_host) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: null argument", v.name);
    if (offsets_host[0] != 0 || offsets_host[n_obj] != n_pairs) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: offsets must run from 0 to n_pairs", v.name);
    for (int k = 0; k < n_obj; ++k)
        if (offsets_host[k + 1] < offsets_host[k]) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: offsets decrease at object %d", v.name, k);
    // every pair count is <= n_pairs < 2^63 / 64 only if n_pairs is sane: bound it before the products below
    if (n_pairs >= (1ll << 31))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "%s limits: samples of all groups < 2^31 (n_pairs=%lld): render the pixel range in bands", v.name, (long long)n_pairs);
    const vl::ScenePlan plan = vl::scene_plan_host(reinterpret_cast<const long long*>(offsets_host), g, v.n_groups);
    if (plan.samples >= (1ll << 31))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "%s limits: samples of all groups < 2^31 (%lld): render the pixel range in bands", v.name, plan.samples);
    for (int i = 0; i < v.n_groups; ++i) {
        if (int rc = check_params(v.groups[i].params, "params", false)) return rc;
        if (!v.groups[i].pe_scale || !v.groups[i].pe_scale->ptr) return fail(VMAPSTEP_ERR_ARGUMENT, "%s: pe_scale of group %d is null", v.name, i);
    }
    if (!boxes || !centers || !offsets || !depth || !color || !opacity || !instance || !overflow ||
        (n_pairs > 0 && (!pairs || !sample_occ || !sample_rgb)))
        return fail(VMAPSTEP_ERR_ARGUMENT, "%s: null argument", v.name);
    if (int rc = check_view_workspace(v, l, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    hipStream_t st = static_cast<hipStream_t>(stream);
    vv::ViewArgs a = view_args(v, g, l, boxes, workspace);
    a.centers = centers;
    a.offsets = const_cast<long long*>(reinterpret_cast<const long long*>(offsets));
    a.pairs = static_cast<vg::Pair*>(pairs); a.cap = n_pairs;
    a.occ = sample_occ; a.rgb = sample_rgb;
    a.depth = depth; a.color = color; a.opacity = opacity; a.instance = instance; a.overflow = overflow;
    for (int i = 0; i < v.n_groups; ++i) { a.g_shift[i] = plan.shift[i]; a.g_per[i] = plan.per[i]; }
    if (int rc = vl::view_emit(a, st)) return rc;
    // the field pass, group by group.  Each launch gets the GROUP's argument block: its objects alone (object index, centres, scales,
    // offsets and images start at the group's first object), its sample count as cam.samples, its plan entries, and occ / rgb placed so
    // that pair * samples addresses the group's section (integer arithmetic: the address of element g_shift of the buffers)
    int k0 = 0;
    for (int i = 0; i < v.n_groups; ++i) {
        const vmapstep_view_group& q = v.groups[i];
        vv::ViewArgs b = a;
        b.n_obj = q.n_obj; b.cam.samples = q.samples;
        b.centers = centers + 3 * k0; b.offsets = a.offsets + k0;
        b.scale = q.pe_scale->ptr; b.scale_so = q.pe_scale->obj_stride;
        b.wimg = static_cast<char*>(workspace) + l.off_img[i];
        b.plan = a.plan + 4 * plan.first[i];
        b.occ = reinterpret_cast<float*>(reinterpret_cast<intptr_t>(sample_occ) + plan.shift[i] * (long long)sizeof(float));
        b.rgb = reinterpret_cast<float*>(reinterpret_cast<intptr_t>(sample_rgb) + 3 * plan.shift[i] * (long long)sizeof(float));
        vk::StepArgs pk;
        std::memset(&pk, 0, sizeof(pk));
        pk.n_obj = q.n_obj; pk.hidden = q.hidden; pk.prep_steps = 0;
        for (int t = 0; t < VMAPSTEP_NUM_FC; ++t) pk.fc[t] = {q.params->fc[t].ptr, q.params->fc[t].obj_stride};
        pk.pe_B = {q.params->pe_B.ptr, q.params->pe_B.obj_stride};
        pk.wimg = reinterpret_cast<float*>(const_cast<char*>(b.wimg));
        if (int rc = vl::view_field(pk, b, plan.entries[i], st)) return rc;
        k0 += q.n_obj;
    }
    return vl::view_composite(a, st);
}

// ---- the single-group hidden-32 entry points: cfg->n_obj objects with cfg->samples samples per hit --------------------------------------
static int check_view_cfg(const vmapstep_view_cfg* c) {
    if (!c) return fail(VMAPSTEP_ERR_ARGUMENT, "view: cfg is null");
    if (c->samples < 1 || c->samples > vv::kViewMaxSamples || c->n_obj < 1 || c->n_obj > vv::kViewMaxObj || c->width < 1 || c->height < 1 ||
        c->width > 16384 || c->height > 16384)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "view limits: 1 <= samples <= %d, 1 <= n_obj <= %d, 1 <= width, height <= 16384 (samples=%d n_obj=%d width=%d height=%d)",
                    vv::kViewMaxSamples, vv::kViewMaxObj, c->samples, c->n_obj, c->width, c->height);
    return check_camera("view", c);
}

static ViewCall one_group(const vmapstep_view_cfg* c, vmapstep_view_group* group, const vmapstep_params* params, const vmapstep_tensor* pe_scale) {
    *group = vmapstep_view_group{32, c->n_obj, c->samples, 0, params, pe_scale};
    return ViewCall{"view", c, group, 1, kViewFrontPlanCap};
}

int vmapstep_view_workspace_bytes(const vmapstep_view_cfg* cfg, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_view_cfg(cfg)) return rc;
    vmapstep_view_group group;
    vl::SceneGroup g[vv::kViewMaxGroups];
    *bytes = view_layout_of(one_group(cfg, &group, nullptr, nullptr), g).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_view_count(const vmapstep_view_cfg* cfg, const float* boxes, int64_t* offsets, void* workspace, size_t workspace_bytes,
                        void* stream) {
    if (int rc = check_view_cfg(cfg)) return rc;
    vmapstep_view_group group;
    return view_count_body(one_group(cfg, &group, nullptr, nullptr), boxes, offsets, workspace, workspace_bytes, stream);
}

int vmapstep_view_render(const vmapstep_view_cfg* cfg, int32_t hidden, const vmapstep_params* params, const vmapstep_tensor* pe_scale,
                         const float* boxes, const float* centers, const int64_t* offsets, const int64_t* offsets_host,
                         void* pairs, int64_t n_pairs, float* sample_occ, float* sample_rgb,
                         float* depth, float* color, float* opacity, int32_t* instance, int32_t* overflow,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (hidden != 32) return fail(VMAPSTEP_ERR_UNSUPPORTED, "view: hidden=%d, the view renderer implements hidden 32 only", hidden);
    if (int rc = check_view_cfg(cfg)) return rc;
    // these fire before the offsets are looked at, the shared body's come after: the order of this entry point's checks stays
    if (n_pairs < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "view: n_pairs=%lld", (long long)n_pairs);
    if (n_pairs * cfg->samples >= (1ll << 31))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "view limits: n_pairs * samples < 2^31 (n_pairs=%lld samples=%d): render the pixel range in bands",
                    (long long)n_pairs, cfg->samples);
    if (int rc = check_params(params, "params", false)) return rc;
    if (!pe_scale || !pe_scale->ptr || !boxes || !centers || !offsets || !offsets_host || !depth || !color || !opacity || !instance || !overflow ||
        (n_pairs > 0 && (!pairs || !sample_occ || !sample_rgb)))
        return fail(VMAPSTEP_ERR_ARGUMENT, "view: null argument");
    vmapstep_view_group group;
    return view_render_body(one_group(cfg, &group, params, pe_scale), boxes, centers, offsets, offsets_host, pairs, n_pairs, sample_occ, sample_rgb,
                            depth, color, opacity, instance, overflow, workspace, workspace_bytes, stream);
}

// ---- the scene entry points: 1 .. VMAPSTEP_VIEW_MAX_GROUPS groups ------------------------------------------------------------------------
static int check_scene(const vmapstep_view_cfg* c, const vmapstep_view_group* groups, int32_t n_groups) {
    if (!c) return fail(VMAPSTEP_ERR_ARGUMENT, "scene view: cfg is null");
    if (n_groups < 1 || n_groups > vv::kViewMaxGroups)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "scene view limits: 1 <= n_groups <= %d (n_groups=%d)", vv::kViewMaxGroups, n_groups);
    if (!groups) return fail(VMAPSTEP_ERR_ARGUMENT, "scene view: groups is null");
    long long total = 0;
    for (int32_t i = 0; i < n_groups; ++i) {
        const vmapstep_view_group& q = groups[i];
        if (q.hidden < 32 || q.hidden > 256 || q.hidden % 32 != 0 || q.samples < 1 || q.samples > vv::kViewMaxSamples || q.n_obj < 1)
            return fail(VMAPSTEP_ERR_UNSUPPORTED, "scene view limits: hidden a multiple of 32 in [32, 256], 1 <= samples <= %d, n_obj >= 1 "
                        "(group %d: hidden=%d samples=%d n_obj=%d)", vv::kViewMaxSamples, (int)i, q.hidden, q.samples, q.n_obj);
        total += q.n_obj;
    }
    if (total > vv::kViewMaxObj || c->width < 1 || c->height < 1 || c->width > 16384 || c->height > 16384)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "scene view limits: objects of all groups <= %d, 1 <= width, height <= 16384 (objects=%lld width=%d height=%d)",
                    vv::kViewMaxObj, total, c->width, c->height);
    return check_camera("scene view", c);
}

int vmapstep_scene_view_workspace_bytes(const vmapstep_view_cfg* cfg, const vmapstep_view_group* groups, int32_t n_groups, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_scene(cfg, groups, n_groups)) return rc;
    vl::SceneGroup g[vv::kViewMaxGroups];
    *bytes = view_layout_of(ViewCall{"scene view", cfg, groups, n_groups, vl::kScenePlanCap}, g).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_scene_view_count(const vmapstep_view_cfg* cfg, const vmapstep_view_group* groups, int32_t n_groups, const float* boxes,
                              int64_t* offsets, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_scene(cfg, groups, n_groups)) return rc;
    return view_count_body(ViewCall{"scene view", cfg, groups, n_groups, vl::kScenePlanCap}, boxes, offsets, workspace, workspace_bytes, stream);
}

int vmapstep_scene_view_render(const vmapstep_view_cfg* cfg, const vmapstep_view_group* groups, int32_t n_groups,
                               const float* boxes, const float* centers, const int64_t* offsets, const int64_t* offsets_host,
                               void* pairs, int64_t n_pairs, float* sample_occ, float* sample_rgb,
                               float* depth, float* color, float* opacity, int32_t* instance, int32_t* overflow,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_scene(cfg, groups, n_groups)) return rc;
    return view_render_body(ViewCall{"scene view", cfg, groups, n_groups, vl::kScenePlanCap}, boxes, centers, offsets, offsets_host, pairs, n_pairs,
                            sample_occ, sample_rgb, depth, color, opacity, instance, overflow, workspace, workspace_bytes, stream);
}

// ---- frame ingest ------------------------------------------------------------------------------------------------------------------
static int check_ingest_ids(int32_t max_ids) {
    if (max_ids < 2 || max_ids > vi::kMaxIds)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "ingest limits: 2 <= max_ids <= %d (max_ids=%d)", vi::kMaxIds, max_ids);
    return VMAPSTEP_OK;
}

int vmapstep_ingest_workspace_bytes(int32_t max_ids, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_ingest_ids(max_ids)) return rc;
    *bytes = vl::ingest_layout(max_ids).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_ingest_frame(const vmapstep_ingest_cfg* cfg, const void* rgb, const void* depth, const void* inst, const void* sem,
                          void* out_rgbx, float* out_depth, int32_t* out_inst, int32_t* rows_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: cfg is null");
    if (!rgb || !depth || !out_rgbx || !out_depth || !out_inst || !rows_out) return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: null argument");
    if (sem && !inst) return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: sem without inst");
    if (cfg->width < 1 || cfg->height < 1 || cfg->n_background < 0 || (cfg->depth_f32 | cfg->label_i32) & ~1)
        return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: width=%d height=%d n_background=%d depth_f32=%d label_i32=%d", cfg->width, cfg->height,
                    cfg->n_background, cfg->depth_f32, cfg->label_i32);
    if (!(cfg->bbox_scale >= 0.0f) || !std::isfinite(cfg->bbox_scale) || !std::isfinite(cfg->depth_scale) || std::isnan(cfg->max_depth))
        return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: bbox_scale must be finite and >= 0, depth_scale finite, max_depth a number");
    if (reinterpret_cast<uintptr_t>(out_rgbx) % 4) return fail(VMAPSTEP_ERR_ARGUMENT, "ingest: out_rgbx must be 4-byte aligned");
    if (cfg->width > vi::kMaxSide || cfg->height > vi::kMaxSide || cfg->n_background > VMAPSTEP_INGEST_MAX_CLASSES)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "ingest limits: width, height <= %d, n_background <= %d (width=%d height=%d n_background=%d)",
                    vi::kMaxSide, VMAPSTEP_INGEST_MAX_CLASSES, cfg->width, cfg->height, cfg->n_background);
    if (int rc = check_ingest_ids(cfg->max_ids)) return rc;
    const size_t need = vl::ingest_layout(cfg->max_ids).bytes;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "ingest workspace must be 256-byte aligned and >= %zu bytes", need);
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::ingest_frame(*cfg, rgb, depth, inst, sem, out_rgbx, out_depth, reinterpret_cast<int*>(out_inst), reinterpret_cast<int*>(rows_out),
                            workspace, static_cast<hipStream_t>(stream));
}

// ---- instance filter ---------------------------------------------------------------------------------------------------------------
static int check_filter_cfg(const vmapstep_filter_cfg* cfg) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "filter: cfg is null");
    if (cfg->width < 1 || cfg->height < 1 || cfg->n_background < 0 || (cfg->depth_f32 | cfg->label_i32) & ~1)
        return fail(VMAPSTEP_ERR_ARGUMENT, "filter: width=%d height=%d n_background=%d depth_f32=%d label_i32=%d", cfg->width, cfg->height,
                    cfg->n_background, cfg->depth_f32, cfg->label_i32);
    if (!std::isfinite(cfg->depth_scale) || std::isnan(cfg->max_depth) || !(cfg->voxel_size > 0.0f) || !std::isfinite(cfg->voxel_size))
        return fail(VMAPSTEP_ERR_ARGUMENT, "filter: depth_scale must be finite, max_depth a number, voxel_size finite and > 0");
    if (cfg->width > vf::kMaxSide || cfg->height > vf::kMaxSide || cfg->n_background > VMAPSTEP_FILTER_MAX_CLASSES)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "filter limits: width, height <= %d, n_background <= %d (width=%d height=%d n_background=%d)",
                    vf::kMaxSide, VMAPSTEP_FILTER_MAX_CLASSES, cfg->width, cfg->height, cfg->n_background);
    if (cfg->max_ids < 2 || cfg->max_ids > vf::kMaxIds || cfg->erode_radius < 0 || cfg->erode_radius > vf::kMaxRadius)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "filter limits: 2 <= max_ids <= %d, 0 <= erode_radius <= %d (max_ids=%d erode_radius=%d)",
                    vf::kMaxIds, vf::kMaxRadius, cfg->max_ids, cfg->erode_radius);
    return VMAPSTEP_OK;
}

static int check_filter_workspace(const vmapstep_filter_cfg* cfg, const void* workspace, size_t workspace_bytes) {
    const size_t need = vl::filter_layout(cfg->max_ids, cfg->width, cfg->height).bytes;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "filter workspace must be 256-byte aligned and >= %zu bytes", need);
    return VMAPSTEP_OK;
}

int vmapstep_filter_workspace_bytes(const vmapstep_filter_cfg* cfg, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_filter_cfg(cfg)) return rc;
    *bytes = vl::filter_layout(cfg->max_ids, cfg->width, cfg->height).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_filter_stats(const vmapstep_filter_cfg* cfg, const void* depth, const void* inst, const void* sem, const float* box_table,
                          int32_t* status, int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !depth || !inst || !sem || !box_table || !status || !rows_out) return fail(VMAPSTEP_ERR_ARGUMENT, "filter_stats: null argument");
    if (int rc = check_filter_cfg(cfg)) return rc;
    if (int rc = check_filter_workspace(cfg, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::filter_stats(*cfg, depth, inst, sem, box_table, reinterpret_cast<int*>(status), reinterpret_cast<int*>(rows_out), workspace,
                            static_cast<hipStream_t>(stream));
}

int vmapstep_filter_emit(const vmapstep_filter_cfg* cfg, const void* depth, const void* inst, const int32_t* status, uint64_t* keys_out,
                         int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !depth || !inst || !status || !keys_out || !rows_out) return fail(VMAPSTEP_ERR_ARGUMENT, "filter_emit: null argument");
    if (int rc = check_filter_cfg(cfg)) return rc;
    if (int rc = check_filter_workspace(cfg, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::filter_emit(*cfg, depth, inst, reinterpret_cast<const int*>(status), reinterpret_cast<unsigned long long*>(keys_out),
                           reinterpret_cast<int*>(rows_out), workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_filter_write(const vmapstep_filter_cfg* cfg, const void* depth, const void* inst, const float* box_table,
                          const int32_t* status, int32_t* labels_out, void* stream) {
    if (!cfg || !depth || !inst || !box_table || !status || !labels_out) return fail(VMAPSTEP_ERR_ARGUMENT, "filter_write: null argument");
    if (int rc = check_filter_cfg(cfg)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::filter_write(*cfg, depth, inst, box_table, reinterpret_cast<const int*>(status), reinterpret_cast<int*>(labels_out),
                            static_cast<hipStream_t>(stream));
}

int vmapstep_voxel_points(const uint64_t* keys, int64_t n_keys, const int64_t* offsets, int32_t n_seg, float voxel_size,
                          float* points, float* bounds, void* stream) {
    if (!keys || !offsets || !points || !bounds) return fail(VMAPSTEP_ERR_ARGUMENT, "voxel_points: null argument");
    if (n_keys < 0 || n_seg < 1 || !(voxel_size > 0.0f) || !std::isfinite(voxel_size))
        return fail(VMAPSTEP_ERR_ARGUMENT, "voxel_points: n_keys=%lld n_seg=%d, voxel_size must be finite and > 0", (long long)n_keys, n_seg);
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::voxel_points(reinterpret_cast<const unsigned long long*>(keys), n_keys, reinterpret_cast<const long long*>(offsets), n_seg,
                            voxel_size, points, bounds, static_cast<hipStream_t>(stream));
}

// ---- instance tracker --------------------------------------------------------------------------------------------------------------
static int check_track_cfg(const vmapstep_track_cfg* cfg) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "track: cfg is null");
    if (cfg->width < 1 || cfg->height < 1 || cfg->n_background < 0 || (cfg->depth_f32 | cfg->label_i32) & ~1)
        return fail(VMAPSTEP_ERR_ARGUMENT, "track: width=%d height=%d n_background=%d depth_f32=%d label_i32=%d", cfg->width, cfg->height,
                    cfg->n_background, cfg->depth_f32, cfg->label_i32);
    if (!std::isfinite(cfg->depth_scale) || std::isnan(cfg->max_depth) || !(cfg->voxel_size > 0.0f) || !std::isfinite(cfg->voxel_size))
        return fail(VMAPSTEP_ERR_ARGUMENT, "track: depth_scale must be finite, max_depth a number, voxel_size finite and > 0");
    if (cfg->width > vf::kMaxSide || cfg->height > vf::kMaxSide || cfg->n_background > VMAPSTEP_FILTER_MAX_CLASSES)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "track limits: width, height <= %d, n_background <= %d (width=%d height=%d n_background=%d)",
                    vf::kMaxSide, VMAPSTEP_FILTER_MAX_CLASSES, cfg->width, cfg->height, cfg->n_background);
    if (cfg->max_det < 1 || cfg->max_det > vt::kMaxDet || cfg->max_pairs < 1 || cfg->max_pairs > vt::kMaxPairs || cfg->max_ids < 2 ||
        cfg->max_ids > vf::kMaxIds || cfg->erode_radius < 0 || cfg->erode_radius > vf::kMaxRadius)
        return fail(VMAPSTEP_ERR_UNSUPPORTED,
                    "track limits: 1 <= max_det <= %d, 1 <= max_pairs <= %d, 2 <= max_ids <= %d, 0 <= erode_radius <= %d (max_det=%d max_pairs=%d "
                    "max_ids=%d erode_radius=%d)", vt::kMaxDet, vt::kMaxPairs, vf::kMaxIds, vf::kMaxRadius, cfg->max_det, cfg->max_pairs,
                    cfg->max_ids, cfg->erode_radius);
    if (cfg->n_pairs > cfg->max_pairs)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "track limits: the frame needs %d pairs, max_pairs = %d", cfg->n_pairs, cfg->max_pairs);
    if (cfg->n_det < 0 || cfg->n_det > cfg->max_det || cfg->n_pairs < 0 || cfg->next_id < 1 || cfg->next_id > cfg->max_ids || cfg->ratio_q < 0)
        return fail(VMAPSTEP_ERR_ARGUMENT, "track: n_det=%d (max_det=%d) n_pairs=%d next_id=%d (max_ids=%d) ratio_q=%d", cfg->n_det, cfg->max_det,
                    cfg->n_pairs, cfg->next_id, cfg->max_ids, cfg->ratio_q);
    return VMAPSTEP_OK;
}

static int check_track_workspace(const vmapstep_track_cfg* cfg, const void* workspace, size_t workspace_bytes) {
    const size_t need = vl::track_layout(cfg->max_det, cfg->max_pairs, cfg->width, cfg->height).bytes;
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % kAlign || workspace_bytes < need)
        return fail(VMAPSTEP_ERR_WORKSPACE, "track workspace must be 256-byte aligned and >= %zu bytes", need);
    return VMAPSTEP_OK;
}

int vmapstep_track_workspace_bytes(const vmapstep_track_cfg* cfg, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_track_cfg(cfg)) return rc;
    *bytes = vl::track_layout(cfg->max_det, cfg->max_pairs, cfg->width, cfg->height).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_track_stats(const vmapstep_track_cfg* cfg, const void* depth, const void* det, const int32_t* meta, const float* box_table,
                         int32_t* status, int32_t* ident, int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !depth || !det || !meta || !box_table || !status || !ident || !rows_out) return fail(VMAPSTEP_ERR_ARGUMENT, "track_stats: null argument");
    if (int rc = check_track_cfg(cfg)) return rc;
    if (int rc = check_track_workspace(cfg, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::track_stats(*cfg, depth, det, reinterpret_cast<const int*>(meta), box_table, reinterpret_cast<int*>(status),
                           reinterpret_cast<int*>(ident), reinterpret_cast<int*>(rows_out), workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_track_emit(const vmapstep_track_cfg* cfg, const void* depth, const void* det, const float* box_table, const int32_t* status,
                        const int32_t* ident, uint64_t* keys_out, int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !depth || !det || !box_table || !status || !ident || !keys_out || !rows_out)
        return fail(VMAPSTEP_ERR_ARGUMENT, "track_emit: null argument");
    if (int rc = check_track_cfg(cfg)) return rc;
    if (int rc = check_track_workspace(cfg, workspace, workspace_bytes)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::track_emit(*cfg, depth, det, box_table, reinterpret_cast<const int*>(status), reinterpret_cast<const int*>(ident),
                          reinterpret_cast<unsigned long long*>(keys_out), reinterpret_cast<int*>(rows_out), workspace,
                          static_cast<hipStream_t>(stream));
}

int vmapstep_track_write(const vmapstep_track_cfg* cfg, const void* depth, const void* det, const float* box_table, const int32_t* status,
                         const int32_t* ident, int32_t* labels_out, void* stream) {
    if (!cfg || !depth || !det || !box_table || !status || !ident || !labels_out) return fail(VMAPSTEP_ERR_ARGUMENT, "track_write: null argument");
    if (int rc = check_track_cfg(cfg)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::track_write(*cfg, depth, det, box_table, reinterpret_cast<const int*>(status), reinterpret_cast<const int*>(ident),
                           reinterpret_cast<int*>(labels_out), static_cast<hipStream_t>(stream));
}

// ---- visibility culling ------------------------------------------------------------------------------------------------------------
static int check_cull_cfg(const vmapstep_cull_cfg* cfg, const float* depth) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "cull: cfg is null");
    if (cfg->width < 1 || cfg->height < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "cull: width=%d height=%d", cfg->width, cfg->height);
    if (cfg->margin < 0 || 2ll * cfg->margin >= cfg->width || 2ll * cfg->margin >= cfg->height)
        return fail(VMAPSTEP_ERR_ARGUMENT, "cull: margin=%d leaves no pixel of %d x %d", cfg->margin, cfg->width, cfg->height);
    if (!(cfg->min_depth >= 0.0f) || !std::isfinite(cfg->min_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "cull: min_depth must be finite and >= 0");
    if (!std::isfinite(cfg->fx) || !std::isfinite(cfg->fy) || !std::isfinite(cfg->cx) || !std::isfinite(cfg->cy) || cfg->fx == 0.0f || cfg->fy == 0.0f)
        return fail(VMAPSTEP_ERR_ARGUMENT, "cull: intrinsics must be finite with fx, fy != 0");
    if (cfg->use_depth && !depth) return fail(VMAPSTEP_ERR_ARGUMENT, "cull: use_depth with a null depth");
    if (cfg->use_depth && !(cfg->occlusion_eps >= 0.0f)) return fail(VMAPSTEP_ERR_ARGUMENT, "cull: occlusion_eps must be a number >= 0");
    return VMAPSTEP_OK;
}

int vmapstep_cull_mark(const float* points, int64_t n_points, const float* depth, const float* t_wc, const int32_t* slots, int32_t n_frames,
                       const vmapstep_cull_cfg* cfg, uint8_t* seen, void* stream) {
    if (int rc = check_cull_cfg(cfg, depth)) return rc;
    if (n_points < 0 || n_points >= (1ll << 31) || n_frames < 0)
        return fail(VMAPSTEP_ERR_ARGUMENT, "cull_mark: n_points=%lld n_frames=%d", (long long)n_points, n_frames);
    if (n_points == 0 || n_frames == 0) return VMAPSTEP_OK;
    if (!points || !t_wc || !seen) return fail(VMAPSTEP_ERR_ARGUMENT, "cull_mark: null argument");
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::cull_mark(*cfg, points, n_points, depth, t_wc, reinterpret_cast<const int*>(slots), n_frames, seen, static_cast<hipStream_t>(stream));
}

static int check_cull_faces(const int32_t* faces, int64_t n_faces, const uint8_t* seen, int64_t n_vertices, int32_t min_seen) {
    if (n_vertices < 0 || n_vertices >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: counts 0 .. 2^31 - 1");
    if (min_seen < 1 || min_seen > 3) return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: min_seen=%d outside 1..3", min_seen);
    if (n_faces > 0 && n_vertices == 0) return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: %lld faces and no vertex", (long long)n_faces);
    if (n_faces > 0 && (!faces || !seen)) return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: null argument");
    return VMAPSTEP_OK;
}

int vmapstep_cull_workspace_bytes(int64_t n_vertices, int64_t n_faces, size_t* bytes) {
    if (!bytes || n_vertices < 0 || n_vertices >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "null / negative argument");
    *bytes = vl::cull_layout(n_vertices, n_faces).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_cull_faces_count(const int32_t* faces, int64_t n_faces, const uint8_t* seen, int64_t n_vertices, int32_t min_seen,
                              int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_cull_faces(faces, n_faces, seen, n_vertices, min_seen)) return rc;
    if (!counts) return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::cull_layout(n_vertices, n_faces).bytes, "cull")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::cull_faces_count(reinterpret_cast<const int*>(faces), n_faces, seen, n_vertices, min_seen, reinterpret_cast<long long*>(counts),
                                workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_cull_faces_emit(const int32_t* faces, int64_t n_faces, const uint8_t* seen, int64_t n_vertices, int32_t min_seen,
                             int32_t* kept_vertices, int64_t n_kept_vertices, int32_t* faces_out, int64_t n_kept_faces,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_cull_faces(faces, n_faces, seen, n_vertices, min_seen)) return rc;
    if (n_kept_vertices < 0 || n_kept_faces < 0 || (n_kept_vertices > 0 && !kept_vertices) || (n_kept_faces > 0 && !faces_out))
        return fail(VMAPSTEP_ERR_ARGUMENT, "cull faces: null argument / negative count");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::cull_layout(n_vertices, n_faces).bytes, "cull")) return rc;
    if (n_faces == 0 || n_kept_faces == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::cull_faces_emit(reinterpret_cast<const int*>(faces), n_faces, seen, n_vertices, min_seen, reinterpret_cast<int*>(kept_vertices),
                               n_kept_vertices, reinterpret_cast<int*>(faces_out), n_kept_faces, workspace, static_cast<hipStream_t>(stream));
}

// ---- mesh components ---------------------------------------------------------------------------------------------------------------
static int check_component_sizes(int64_t n_vertices, int64_t n_faces) {
    if (n_vertices < 0 || n_vertices >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "components: n_vertices=%lld n_faces=%lld outside 0 .. 2^31 - 1", (long long)n_vertices, (long long)n_faces);
    return VMAPSTEP_OK;
}

int vmapstep_components_workspace_bytes(int64_t n_vertices, int64_t n_faces, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "components: null argument");
    if (int rc = check_component_sizes(n_vertices, n_faces)) return rc;
    *bytes = vl::component_layout(n_vertices, n_faces).bytes;
    return VMAPSTEP_OK;
}

int vmapstep_components_label(const int32_t* faces, int64_t n_faces, int64_t n_vertices, int32_t* labels, int64_t* counts, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (int rc = check_component_sizes(n_vertices, n_faces)) return rc;
    if (!counts || (n_faces > 0 && !faces) || (n_vertices > 0 && !labels)) return fail(VMAPSTEP_ERR_ARGUMENT, "components_label: null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::component_layout(n_vertices, n_faces).bytes, "components")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::components_label(reinterpret_cast<const int*>(faces), n_faces, n_vertices, reinterpret_cast<int*>(labels),
                                reinterpret_cast<long long*>(counts), workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_components_stats(const float* vertices, const int32_t* faces, int64_t n_faces, const int32_t* labels, int64_t n_vertices,
                              int64_t n_components, int32_t* comp_vertices, int64_t* comp_faces, int64_t* comp_area_q, void* stream) {
    if (int rc = check_component_sizes(n_vertices, n_faces)) return rc;
    if (n_components < 0 || n_components > n_vertices)
        return fail(VMAPSTEP_ERR_ARGUMENT, "components_stats: n_components=%lld outside [0, n_vertices=%lld]", (long long)n_components, (long long)n_vertices);
    if ((n_faces > 0 && !faces) || (n_vertices > 0 && !labels) || (n_components > 0 && (!comp_vertices || !comp_faces || !comp_area_q)))
        return fail(VMAPSTEP_ERR_ARGUMENT, "components_stats: null argument");
    if (n_components == 0) return VMAPSTEP_OK;             // no row to write (n_vertices == 0 among them)
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::components_stats(vertices, reinterpret_cast<const int*>(faces), n_faces, reinterpret_cast<const int*>(labels), n_vertices, n_components,
                                reinterpret_cast<int*>(comp_vertices), reinterpret_cast<long long*>(comp_faces),
                                reinterpret_cast<long long*>(comp_area_q), static_cast<hipStream_t>(stream));
}

// ---- mesh rasteriser ----------------------------------------------------------------------------------------------------------------
static int check_raster_cfg(const vmapstep_raster_cfg* cfg) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: cfg is null");
    if (cfg->width < 1 || cfg->height < 1 || cfg->width > 16384 || cfg->height > 16384)
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster: width=%d height=%d outside 1 .. 16384", cfg->width, cfg->height);
    if (!(cfg->min_depth > 0.0f) || !std::isfinite(cfg->min_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: min_depth must be finite and > 0");
    if (std::isnan(cfg->max_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: max_depth is not a number");
    if (!std::isfinite(cfg->fx) || !std::isfinite(cfg->fy) || !std::isfinite(cfg->cx) || !std::isfinite(cfg->cy) || cfg->fx == 0.0f || cfg->fy == 0.0f)
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster: intrinsics must be finite with fx, fy != 0");
    return VMAPSTEP_OK;
}

static int check_raster_sizes(int64_t n_vertices, int64_t n_faces, int32_t n_views) {
    if (n_vertices < 0 || n_vertices >= (1ll << 31) || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster: n_vertices=%lld n_faces=%lld outside 0 .. 2^31 - 1", (long long)n_vertices, (long long)n_faces);
    if (n_views < 1 || n_views > 65535) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: n_views=%d outside 1 .. 65535", n_views);
    if (n_faces > 0 && n_vertices == 0) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: %lld faces and no vertex", (long long)n_faces);
    return VMAPSTEP_OK;
}

int vmapstep_raster_workspace_bytes(int64_t n_faces, int32_t n_views, int64_t large_cap, size_t* workspace_bytes, size_t* large_bytes) {
    if (!workspace_bytes || !large_bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "raster: null argument");
    if (int rc = check_raster_sizes(0, 0, n_views)) return rc;
    if (n_faces < 0 || n_faces >= (1ll << 31) || large_cap < 0 || large_cap >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster: n_faces=%lld large_cap=%lld outside 0 .. 2^31 - 1", (long long)n_faces, (long long)large_cap);
    const vl::RasterLayout l = vl::raster_layout(n_faces, n_views, large_cap);
    *workspace_bytes = l.bytes;
    *large_bytes = l.large_bytes;
    return VMAPSTEP_OK;
}

int vmapstep_raster_count(const vmapstep_raster_cfg* cfg, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                          const float* t_wc, const int32_t* slots, int32_t n_views, uint64_t* keys, int32_t* dropped, int64_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_raster_cfg(cfg)) return rc;
    if (int rc = check_raster_sizes(n_vertices, n_faces, n_views)) return rc;
    if (!t_wc || !keys || !dropped || !counts || (n_faces > 0 && (!faces || !vertices))) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_count: null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::raster_layout(n_faces, n_views, 0).bytes, "raster")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::raster_count(*cfg, vertices, n_vertices, reinterpret_cast<const int*>(faces), n_faces, t_wc, reinterpret_cast<const int*>(slots), n_views,
                            reinterpret_cast<unsigned long long*>(keys), reinterpret_cast<int*>(dropped), reinterpret_cast<long long*>(counts),
                            workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_raster_draw(const vmapstep_raster_cfg* cfg, const float* vertices, int64_t n_vertices, const int32_t* faces, int64_t n_faces,
                         const float* t_wc, const int32_t* slots, int32_t n_views, uint64_t* keys, int64_t n_large, int64_t n_pairs,
                         void* large, int64_t large_cap, size_t large_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_raster_cfg(cfg)) return rc;
    if (int rc = check_raster_sizes(n_vertices, n_faces, n_views)) return rc;
    if (n_large < 0 || n_pairs < 0 || large_cap < 0 || large_cap >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster_draw: n_large=%lld n_pairs=%lld large_cap=%lld", (long long)n_large, (long long)n_pairs, (long long)large_cap);
    if (n_large > large_cap) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_draw: large_cap=%lld is too small for %lld large faces", (long long)large_cap, (long long)n_large);
    if (n_large == 0 && n_pairs > 0) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_draw: %lld pairs of no large face", (long long)n_pairs);
    if (n_large > n_faces * (int64_t)n_views) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_draw: n_large=%lld exceeds views x faces", (long long)n_large);
    if (!t_wc || !keys || (n_faces > 0 && (!faces || !vertices))) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_draw: null argument");
    if (int rc = check_eval_workspace(workspace, workspace_bytes, vl::raster_layout(n_faces, n_views, 0).bytes, "raster")) return rc;
    if (n_large == 0 || n_pairs == 0) return VMAPSTEP_OK;  // nothing to draw: nothing enqueued
    if (int rc = check_eval_workspace(large, large_bytes, vl::raster_layout(n_faces, n_views, large_cap).large_bytes, "raster large-face")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::raster_draw(*cfg, vertices, n_vertices, reinterpret_cast<const int*>(faces), n_faces, t_wc, reinterpret_cast<const int*>(slots), n_views,
                           reinterpret_cast<unsigned long long*>(keys), n_large, n_pairs, large, large_cap, workspace, static_cast<hipStream_t>(stream));
}

int vmapstep_raster_resolve(const uint64_t* keys, int64_t n_pixels, float* depth, int32_t* face, const int32_t* face_labels, int64_t n_faces,
                            int32_t* label, uint8_t* face_seen, void* stream) {
    if (n_pixels < 0 || n_faces < 0 || n_faces >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "raster_resolve: n_pixels=%lld n_faces=%lld", (long long)n_pixels, (long long)n_faces);
    if (label && !face_labels) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_resolve: label without face_labels");
    if (n_pixels == 0) return VMAPSTEP_OK;
    if (!keys || !depth || !face) return fail(VMAPSTEP_ERR_ARGUMENT, "raster_resolve: null argument");
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::raster_resolve(reinterpret_cast<const unsigned long long*>(keys), n_pixels, depth, reinterpret_cast<int*>(face),
                              reinterpret_cast<const int*>(face_labels), n_faces, reinterpret_cast<int*>(label), face_seen, static_cast<hipStream_t>(stream));
}

int vmapstep_depth_compare(const float* a, const float* b, int32_t n_views, int64_t pixels_per_view, int64_t* out, void* stream) {
    if (n_views < 1 || n_views > 65535 || pixels_per_view < 1 || pixels_per_view >= (1ll << 31))
        return fail(VMAPSTEP_ERR_ARGUMENT, "depth_compare: n_views=%d (1 .. 65535) pixels_per_view=%lld (1 .. 2^31 - 1)", n_views, (long long)pixels_per_view);
    if (!a || !b || !out) return fail(VMAPSTEP_ERR_ARGUMENT, "depth_compare: null argument");
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::depth_compare(a, b, n_views, pixels_per_view, reinterpret_cast<long long*>(out), static_cast<hipStream_t>(stream));
}

// ---- depth tracker -----------------------------------------------------------------------------------------------------------------
static int check_icp_cfg(const vmapstep_icp_cfg* cfg, bool track) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "icp: cfg is null");
    if (cfg->width < 1 || cfg->height < 1 || cfg->levels < 1 || cfg->levels > VMAPSTEP_ICP_MAX_LEVELS || cfg->min_inliers < 0 || cfg->grid_cap < 0)
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp: width=%d height=%d levels=%d (1 .. %d) min_inliers=%d grid_cap=%d", cfg->width, cfg->height,
                    cfg->levels, VMAPSTEP_ICP_MAX_LEVELS, cfg->min_inliers, cfg->grid_cap);
    const float cam[4] = {cfg->fx, cfg->fy, cfg->cx, cfg->cy};
    for (float v : cam)
        if (!std::isfinite(v)) return fail(VMAPSTEP_ERR_ARGUMENT, "icp: the camera must be finite");
    if (!(cfg->fx > 0.0f && cfg->fy > 0.0f)) return fail(VMAPSTEP_ERR_ARGUMENT, "icp: fx and fy must be > 0");
    if (!(cfg->min_depth >= 0.0f) || !std::isfinite(cfg->max_depth) || !(cfg->max_depth > cfg->min_depth))
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp: 0 <= min_depth < max_depth < inf");
    if (!(cfg->band >= 0.0f) || !std::isfinite(cfg->band) || !(cfg->dist_thresh >= 0.0f) || !std::isfinite(cfg->dist_thresh) || !std::isfinite(cfg->cos_thresh))
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp: band and dist_thresh must be finite and >= 0, cos_thresh finite");
    if (!(cfg->damping >= 0.0) || !std::isfinite(cfg->damping) || !(cfg->pivot_rel >= 0.0) || !std::isfinite(cfg->pivot_rel) || !(cfg->eps >= 0.0) ||
        !std::isfinite(cfg->eps))
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp: damping, pivot_rel and eps must be finite and >= 0");
    if (track)
        for (int l = 0; l < cfg->levels; ++l)
            if (cfg->iterations[l] < 1 || cfg->iterations[l] > VMAPSTEP_ICP_MAX_ITERATIONS)
                return fail(VMAPSTEP_ERR_ARGUMENT, "icp: iterations[%d]=%d (1 .. %d)", l, cfg->iterations[l], VMAPSTEP_ICP_MAX_ITERATIONS);
    if ((long long)cfg->width * cfg->height > VMAPSTEP_ICP_MAX_PIXELS)
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "icp limits: width * height <= %d, the bound under which the integer sums cannot overflow (width=%d height=%d)",
                    VMAPSTEP_ICP_MAX_PIXELS, cfg->width, cfg->height);
    return VMAPSTEP_OK;
}

static int check_icp_maps(const void* maps, const char* what) {
    if (!maps) return fail(VMAPSTEP_ERR_ARGUMENT, "icp: %s is null", what);
    if (reinterpret_cast<uintptr_t>(maps) % 16) return fail(VMAPSTEP_ERR_WORKSPACE, "icp: %s must be 16-byte aligned", what);
    return VMAPSTEP_OK;
}

int vmapstep_icp_maps_bytes(const vmapstep_icp_cfg* cfg, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "bytes is null");
    if (int rc = check_icp_cfg(cfg, false)) return rc;
    *bytes = (size_t)vl::icp_layout(cfg->width, cfg->height, cfg->levels).entries * 16;
    return VMAPSTEP_OK;
}

int vmapstep_icp_pyramid(const vmapstep_icp_cfg* cfg, const float* depth, void* maps, void* stream) {
    if (int rc = check_icp_cfg(cfg, false)) return rc;
    if (!depth || reinterpret_cast<uintptr_t>(depth) % 4) return fail(VMAPSTEP_ERR_ARGUMENT, "icp_pyramid: depth is null or misaligned");
    if (int rc = check_icp_maps(maps, "maps")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::icp_pyramid(*cfg, depth, maps, static_cast<hipStream_t>(stream));
}

int vmapstep_icp_sums(const vmapstep_icp_cfg* cfg, const void* src_maps, const void* model_maps, int32_t level, const double* t_sm,
                      int64_t* sums, void* stream) {
    if (int rc = check_icp_cfg(cfg, false)) return rc;
    if (level < 0 || level >= cfg->levels) return fail(VMAPSTEP_ERR_ARGUMENT, "icp_sums: level=%d (levels=%d)", level, cfg->levels);
    if (!t_sm || !sums || (reinterpret_cast<uintptr_t>(t_sm) | reinterpret_cast<uintptr_t>(sums)) % 8)
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp_sums: t_sm or sums is null or misaligned");
    if (int rc = check_icp_maps(src_maps, "src_maps")) return rc;
    if (int rc = check_icp_maps(model_maps, "model_maps")) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::icp_sums(*cfg, src_maps, model_maps, level, t_sm, reinterpret_cast<long long*>(sums), static_cast<hipStream_t>(stream));
}

int vmapstep_icp_track(const vmapstep_icp_cfg* cfg, const void* src_maps, const void* model_maps, double* pose, double* log,
                       int64_t* sums_log, double* pose_log, void* state, void* stream) {
    if (int rc = check_icp_cfg(cfg, true)) return rc;
    if (!pose || !log || !sums_log || !pose_log ||
        (reinterpret_cast<uintptr_t>(pose) | reinterpret_cast<uintptr_t>(log) | reinterpret_cast<uintptr_t>(sums_log) | reinterpret_cast<uintptr_t>(pose_log)) % 8)
        return fail(VMAPSTEP_ERR_ARGUMENT, "icp_track: pose, log, sums_log or pose_log is null or misaligned");
    if (int rc = check_icp_maps(src_maps, "src_maps")) return rc;
    if (int rc = check_icp_maps(model_maps, "model_maps")) return rc;
    if (!state || reinterpret_cast<uintptr_t>(state) % kAlign) return fail(VMAPSTEP_ERR_WORKSPACE, "icp_track: state must be 256-byte aligned");
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::icp_track(*cfg, src_maps, model_maps, pose, log, reinterpret_cast<long long*>(sums_log), pose_log, state, static_cast<hipStream_t>(stream));
}

// ---- TSDF fusion -------------------------------------------------------------------------------------------------------------------
int vmapstep_tsdf_integrate(const vmapstep_tsdf_cfg* cfg, float* tsdf, float* weight, float* color, const float* depth, const uint8_t* rgbx,
                            const int32_t* inst, const float* poses, const int32_t* slots, int32_t n_frames, void* stream) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: cfg is null");
    if (!tsdf || !weight || !depth || !poses) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: tsdf, weight, depth or poses is null");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(tsdf) | at(weight) | at(depth) | at(poses) | at(inst) | at(slots) | at(rgbx)) % 4 || at(color) % 16)
        return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: a pointer is not aligned to its element (color: 16 bytes)");
    if (color && !rgbx) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: a colour volume needs rgbx");
    if (cfg->obj_id >= 0 && !inst) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: obj_id=%d needs inst", cfg->obj_id);
    if (!(cfg->trunc > 0.0f) || !std::isfinite(cfg->trunc)) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: trunc must be finite and > 0");
    if (!(cfg->max_weight >= 1.0f)) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: max_weight must be >= 1");
    if (!(cfg->max_depth > cfg->min_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: max_depth must be > min_depth");
    if (n_frames < 0) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: n_frames=%d", n_frames);
    for (int e = 0; e < 12; ++e)
        if (!std::isfinite(cfg->affine[e])) return fail(VMAPSTEP_ERR_ARGUMENT, "tsdf: the affine is not finite");
    vmapstep_cull_cfg cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = cfg->fx; cam.fy = cfg->fy; cam.cx = cfg->cx; cam.cy = cfg->cy; cam.min_depth = cfg->min_depth;
    cam.width = cfg->width; cam.height = cfg->height; cam.margin = cfg->margin;
    if (int rc = check_cull_cfg(&cam, depth)) return rc;
    if (int rc = check_mesh_shape(cfg->nx, cfg->ny, cfg->nz)) return rc;
    if (n_frames == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::tsdf_integrate(*cfg, tsdf, weight, color, depth, rgbx, reinterpret_cast<const int*>(inst), poses, reinterpret_cast<const int*>(slots),
                              n_frames, static_cast<hipStream_t>(stream));
}

// ---- TSDF ray cast -----------------------------------------------------------------------------------------------------------------
static size_t bricks_count(int32_t nx, int32_t ny, int32_t nz) {
    return (size_t)rc::brick_dim(nx) * rc::brick_dim(ny) * rc::brick_dim(nz);
}

int vmapstep_tsdf_bricks_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes) {
    if (!bytes) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: bytes is null");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    *bytes = (bricks_count(nx, ny, nz) + 15) / 16 * 16;
    return VMAPSTEP_OK;
}

int vmapstep_tsdf_bricks(int32_t nx, int32_t ny, int32_t nz, float min_weight, const float* tsdf, const float* weight, uint8_t* bricks,
                         void* stream) {
    if (!tsdf || !weight || !bricks) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: tsdf, weight or bricks is null");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(tsdf) | at(weight)) % 4 || at(bricks) % 16)
        return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: a pointer is not aligned to its element (bricks: 16 bytes)");
    if (!(min_weight > 0.0f) || !std::isfinite(min_weight)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: min_weight must be finite and > 0");
    if (int rc = check_mesh_shape(nx, ny, nz)) return rc;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::tsdf_bricks(nx, ny, nz, min_weight, tsdf, weight, bricks, static_cast<hipStream_t>(stream));
}

int vmapstep_tsdf_raycast(const vmapstep_raycast_cfg* cfg, const float* tsdf, const float* weight, const float* color, const uint8_t* bricks,
                          const float* views, int32_t n_views, float* depth, uint8_t* status, float* normal, uint8_t* color_out, void* stream) {
    if (!cfg) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: cfg is null");
    if (!tsdf || !weight || !views || !depth || !status) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: tsdf, weight, views, depth or status is null");
    const auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    if ((at(tsdf) | at(weight) | at(views) | at(depth) | at(normal) | at(color_out)) % 4 || (at(color) | at(bricks)) % 16)
        return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: a pointer is not aligned to its element (color, bricks: 16 bytes; color_out: 4)");
    if (color_out && !color) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: color_out needs a colour volume");
    if (!(cfg->step > 0.0f) || !std::isfinite(cfg->step)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: step must be finite and > 0");
    if (!(cfg->min_weight > 0.0f) || !std::isfinite(cfg->min_weight)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: min_weight must be finite and > 0");
    if (!(cfg->fx > 0.0f) || !(cfg->fy > 0.0f) || !std::isfinite(cfg->fx) || !std::isfinite(cfg->fy) || !std::isfinite(cfg->cx) || !std::isfinite(cfg->cy))
        return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: the camera must be finite with fx, fy > 0");
    if (!(cfg->min_depth >= 0.0f) || !std::isfinite(cfg->min_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: min_depth must be finite and >= 0");
    if (!(cfg->max_depth > cfg->min_depth)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: max_depth must be > min_depth");
    if (cfg->max_steps < 1 || cfg->max_steps >= rc::kMaxStepsLimit) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: max_steps=%d outside 1 .. 2^24 - 1", cfg->max_steps);
    if (cfg->width < 1 || cfg->height < 1 || (long long)cfg->width * cfg->height >= (1ll << 31) / 12)
        return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: width=%d height=%d", cfg->width, cfg->height);
    for (int e = 0; e < 9; ++e)
        if (!std::isfinite(cfg->normal_map[e])) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: normal_map is not finite");
    if (n_views < 0 || (long long)n_views * cfg->width * cfg->height >= (1ll << 40)) return fail(VMAPSTEP_ERR_ARGUMENT, "raycast: n_views=%d", n_views);
    if (int rc = check_mesh_shape(cfg->nx, cfg->ny, cfg->nz)) return rc;
    if (n_views == 0) return VMAPSTEP_OK;
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::tsdf_raycast(*cfg, tsdf, weight, color, (cfg->flags & VMAPSTEP_RAYCAST_IGNORE_BRICKS) ? nullptr : bricks, (int)bricks_count(cfg->nx, cfg->ny, cfg->nz),
                            views, n_views, depth, status, normal, color_out, static_cast<hipStream_t>(stream));
}

int vmapstep_sample_workspace_bytes(int32_t n_obj, size_t* bytes) {
    if (!bytes || n_obj < 1) return fail(VMAPSTEP_ERR_ARGUMENT, "null / non-positive argument");
    *bytes = align_up((size_t)n_obj * sizeof(int));
    return VMAPSTEP_OK;
}

static int sample_frame_impl(const vmapstep_sample_cfg* cfg, const vmapstep_sample_object* objects_device, int32_t n_obj,
                             float* pcs, float* ray_o, float* ray_d, float* center_out,
                             float* z, float* gt_depth, float* gt_rgb, uint8_t* sem, uint8_t* depth_mask,
                             uint64_t seed, uint32_t frame_counter, const vmapstep_sample_randoms* test_randoms,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !objects_device || !z || !gt_depth || !gt_rgb || !sem || !depth_mask)
        return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    if (!pcs && !(ray_o && ray_d)) return fail(VMAPSTEP_ERR_ARGUMENT, "neither pcs nor (ray_o, ray_d) given");
    if ((ray_o == nullptr) != (ray_d == nullptr)) return fail(VMAPSTEP_ERR_ARGUMENT, "ray_o and ray_d go together");
    const int S = cfg->n_bins_cam2surface + cfg->n_bins;
    const long long FP = (long long)cfg->frames * cfg->samples_per_frame;
    if (n_obj < 1 || cfg->frames < 1 || cfg->samples_per_frame < 1 || cfg->n_bins_cam2surface < 1 || cfg->n_bins < 1)
        return fail(VMAPSTEP_ERR_ARGUMENT, "bad sampler shape");
    if (S > vs::kMaxS || cfg->n_bins > 16 || cfg->width > 4095 || cfg->height > 4095 || FP > (1 << 24))
        return fail(VMAPSTEP_ERR_UNSUPPORTED, "sampler limits: S<=32, n_bins<=16, W,H<=4095, F*P<=2^24");
    vs::SampleArgs a;
    std::memset(&a, 0, sizeof(a));
    a.objs = reinterpret_cast<const vs::SampleObject*>(objects_device);
    a.n_obj = n_obj; a.W = cfg->width; a.H = cfg->height; a.F = cfg->frames; a.P = cfg->samples_per_frame;
    a.n1 = cfg->n_bins_cam2surface; a.n2 = cfg->n_bins;
    a.fx = cfg->fx; a.fy = cfg->fy; a.cx = cfg->cx; a.cy = cfg->cy;
    a.min_bound = cfg->min_depth; a.eps = cfg->surface_eps; a.stop_eps = cfg->stop_eps;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32); a.frame_counter = frame_counter;
    if (test_randoms) {
        a.rnd.kf_ids = test_randoms->kf_ids; a.rnd.u_w = test_randoms->u_w; a.rnd.u_h = test_randoms->u_h;
        a.rnd.u_z = test_randoms->u_z; a.rnd.g_z = test_randoms->g_z;
    }
    a.pcs = pcs; a.z = z; a.gt_depth = gt_depth; a.gt_rgb = gt_rgb; a.sem = sem; a.depth_mask = depth_mask;
    a.ray_o = ray_o; a.ray_d = ray_d; a.center_out = center_out;
    if (workspace) {
        // split form: as many workgroups per object as fill the chip, at most one ray per thread
        if (reinterpret_cast<uintptr_t>(workspace) % sizeof(int) || workspace_bytes < (size_t)n_obj * sizeof(int))
            return fail(VMAPSTEP_ERR_WORKSPACE, "sampler workspace: need %zu bytes (vmapstep_sample_workspace_bytes)", (size_t)n_obj * sizeof(int));
        const long long per_obj_max = (FP + vs::kWG - 1) / vs::kWG;
        long long ns = std::max(1, 512 / n_obj);
        if (ns > per_obj_max) ns = per_obj_max;
        if (ns > 1) { a.nsplit = (int)ns; a.obj_max = static_cast<int*>(workspace); }
    }
    VMAPSTEP_ON_STREAM_DEVICE(stream);
    return vl::sample_frame(a, n_obj, FP, static_cast<hipStream_t>(stream));
}

int vmapstep_sample_frame(const vmapstep_sample_cfg* cfg, const vmapstep_sample_object* objects_device, int32_t n_obj,
                          float* pcs, float* z, float* gt_depth, float* gt_rgb, uint8_t* sem, uint8_t* depth_mask,
                          uint64_t seed, uint32_t frame_counter, const vmapstep_sample_randoms* test_randoms,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!pcs) return fail(VMAPSTEP_ERR_ARGUMENT, "null argument");
    return sample_frame_impl(cfg, objects_device, n_obj, pcs, nullptr, nullptr, nullptr, z, gt_depth, gt_rgb, sem, depth_mask, seed,
                             frame_counter, test_randoms, workspace, workspace_bytes, stream);
}

int vmapstep_sample_frame_rays(const vmapstep_sample_cfg* cfg, const vmapstep_sample_object* objects_device, int32_t n_obj,
                               float* ray_o, float* ray_d, float* center, float* pcs,
                               float* z, float* gt_depth, float* gt_rgb, uint8_t* sem, uint8_t* depth_mask,
                               uint64_t seed, uint32_t frame_counter, const vmapstep_sample_randoms* test_randoms,
                               void* workspace, size_t workspace_bytes, void* stream) {
    if (!ray_o || !ray_d) return fail(VMAPSTEP_ERR_ARGUMENT, "ray_o / ray_d are required");
    return sample_frame_impl(cfg, objects_device, n_obj, pcs, ray_o, ray_d, center, z, gt_depth, gt_rgb, sem, depth_mask, seed,
                             frame_counter, test_randoms, workspace, workspace_bytes, stream);
}

}  // extern "C"
