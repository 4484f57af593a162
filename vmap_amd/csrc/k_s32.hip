// k_s32.hip - hidden 32 on the bf16 matrix pipe with split operands (split_kernels.h): step_prep_s32, step_main_s32,
// step_finalize_s32.  The default path of BASELINE configs[1] / [3].  gfx950 only.
#include "launch.h"
#include "split_kernels.h"

namespace vl {

namespace {
template <bool BWD, bool MULTI, bool STAMPS, bool W3, bool B6 = false, bool PV = false, bool OL = false>
int main_v(const vk::StepArgs& a, hipStream_t st) {
    auto kern = vk::step_main_s32<BWD, MULTI, STAMPS, W3, B6, PV, OL>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), vk::Img32s::LDS_BYTES, "step_main_s32")) return rc;
    const int grid = a.xcd_affine ? 8 * ((a.n_obj + 7) / 8) * a.NW : a.n_obj * a.NW;
    VL_LAUNCH_MAIN(kern, dim3(grid), dim3(vk::kWG), vk::Img32s::LDS_BYTES, st, a);
    return launched("step_main_s32");
}
#ifdef VMAPSTEP_AB
template <bool MULTI, bool W3, bool B6>
int main_of(const vk::StepArgs& a, hipStream_t st) {
    auto kern = vk::step_main_s32_of<MULTI, W3, B6>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), vk::Img32s::LDS_BYTES, "step_main_s32")) return rc;
    const int grid = a.xcd_affine ? 8 * ((a.n_obj + 7) / 8) * a.NW : a.n_obj * a.NW;
    VL_LAUNCH_MAIN(kern, dim3(grid), dim3(vk::kWG), vk::Img32s::LDS_BYTES, st, a);
    return launched("step_main_s32");
}
template <bool MULTI, bool STAMPS, bool W3, bool B6>
int main_ob(const vk::StepArgs& a, hipStream_t st) {
    auto kern = vk::step_main_s32_ob<MULTI, STAMPS, W3, B6>;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), vk::Img32s::LDS_BYTES, "step_main_s32")) return rc;
    const int grid = a.xcd_affine ? 8 * ((a.n_obj + 7) / 8) * a.NW : a.n_obj * a.NW;
    VL_LAUNCH_MAIN(kern, dim3(grid), dim3(vk::kWG), vk::Img32s::LDS_BYTES, st, a);
    return launched("step_main_s32");
}
#endif
template <bool BWD, bool STAMPS>
int main_bs(const vk::StepArgs& a, hipStream_t st) {
    const bool multi = a.NW < a.NG;
#ifdef VMAPSTEP_AB
    if (a.ab_flags & 8) {                    // tuning.ws_flags bit 6: the former backward (training instantiations; phase stamps: float32 weights, three products, one pass)
        if constexpr (BWD) {
            if (!(a.ab_flags & 7)) {
                if constexpr (STAMPS) {
                    if (!a.weights_bf16 && !a.bwd6 && !multi) return main_ob<false, true, true, false>(a, st);
                } else {
                    if (a.weights_bf16) return multi ? main_ob<true, false, false, false>(a, st) : main_ob<false, false, false, false>(a, st);
                    if (a.bwd6) return multi ? main_ob<true, false, true, true>(a, st) : main_ob<false, false, true, true>(a, st);
                    return multi ? main_ob<true, false, true, false>(a, st) : main_ob<false, false, true, false>(a, st);
                }
            }
        }
        return fail(-2, "tuning.ws_flags bit 6 (the former backward of step_main_s32): training steps without bit 3, 4 or 5; phase stamps with float32 weights, the three-product backward and one pass per workgroup only");
    }
    if (a.ab_flags & 4) {                    // tuning.ws_flags bit 5: the former order of the front (training instantiations)
        if constexpr (BWD && !STAMPS) {
            if (!(a.ab_flags & 3)) {
                if (a.weights_bf16) return multi ? main_of<true, false, false>(a, st) : main_of<false, false, false>(a, st);
                if (a.bwd6) return multi ? main_of<true, true, true>(a, st) : main_of<false, true, true>(a, st);
                return multi ? main_of<true, true, false>(a, st) : main_of<false, true, false>(a, st);
            }
        }
        return fail(-2, "tuning.ws_flags bit 5 (the former front of step_main_s32): training steps without phase stamps, bit 3 or bit 4");
    }
    if (a.ab_flags & 2) {                    // tuning.ws_flags bit 4: the former order of the global loads (training instantiations, three-product backward)
        if constexpr (BWD && !STAMPS) {
            if (!a.bwd6 && !(a.ab_flags & 1)) {
                if (a.weights_bf16) return multi ? main_v<true, true, false, false, false, false, true>(a, st) : main_v<true, false, false, false, false, false, true>(a, st);
                return multi ? main_v<true, true, false, true, false, false, true>(a, st) : main_v<true, false, false, true, false, false, true>(a, st);
            }
        }
        return fail(-2, "tuning.ws_flags bit 4 (the former load order of step_main_s32): training steps without phase stamps, bit 3 or the six-product backward");
    }
#endif
    if (a.weights_bf16) return multi ? main_v<BWD, true, STAMPS, false>(a, st) : main_v<BWD, false, STAMPS, false>(a, st);
    if constexpr (BWD && !STAMPS) {          // the six-product backward (tuning.kernel = VMAPSTEP_KERNEL_S32_BWD6): training instantiations only
        if (a.bwd6) return multi ? main_v<true, true, false, true, true>(a, st) : main_v<true, false, false, true, true>(a, st);
#ifdef VMAPSTEP_AB
        if (a.ab_flags & 1) return multi ? main_v<true, true, false, true, false, true>(a, st) : main_v<true, false, false, true, false, true>(a, st);
#endif
    }
    return multi ? main_v<BWD, true, STAMPS, true>(a, st) : main_v<BWD, false, STAMPS, true>(a, st);
}
}  // namespace

int main_s32(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st) {
#ifdef VMAPSTEP_AB
    if (stamps) return main_bs<true, true>(a, st);
#else
    if (stamps) return fail(-2, "this kernel form ships in the measurement build only (tests/tools/libvmapstep_ab.so: phase stamps and A/B forms no automatic plan launches)");
#endif
    return bwd ? main_bs<true, false>(a, st) : main_bs<false, false>(a, st);
}

int prep_s32(const vk::StepArgs& a, int n_steps, hipStream_t st) {
    hipLaunchKernelGGL(vk::step_prep_s32<>, dim3(n_steps + a.n_obj * vk::kSplitPackBlocks), dim3(vk::kWG), 3 * vk::kWG * sizeof(int), st, a);
    return launched("step_prep_s32");
}

int finalize_s32(const vk::FinalizeArgs& f, const vk::FinalizeHot& h, int grid, hipStream_t st) {
    vk::FinalizeArgs g = f;
    const size_t lds = vk::loss_lds_bytes(f.n_obj, f.NW);
    g.loss_stage = vk::loss_stage_cap(lds);
    hipLaunchKernelGGL(vk::step_finalize_s32<>, dim3(grid), dim3(vk::kWG), lds, st, g, h);
    return launched("step_finalize_s32");
}

}  // namespace vl
