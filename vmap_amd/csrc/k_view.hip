// k_view.hip - view rendering (view_kernels.h): the boxes every pixel's ray crosses as count -> scan -> emit, the launch plan of the
// segmented field kernel (which k_misc.hip launches, next to the parameter pack) and the per-pixel composite.  gfx950 only.
#include "launch.h"
#include "view_kernels.h"

namespace vl {

int view_count(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb > 0) {
        hipLaunchKernelGGL(vv::view_count, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
        if (int rc = launched("view_count")) return rc;
    }
    hipLaunchKernelGGL(vv::view_scan, dim3(1), dim3(vv::kViewScanWG), 0, st, a);
    return launched("view_scan");
}

int view_emit(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb > 0 && a.cap > 0) {
        hipLaunchKernelGGL(vv::view_emit, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
        if (int rc = launched("view_emit")) return rc;
    }
    hipError_t e = hipMemsetAsync(a.plan, 0xff, (size_t)kViewPlanCap * 4 * sizeof(int), st);      // no entry: object -1
    if (e != hipSuccess) return fail(-4, "hipMemsetAsync(view plan): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(vv::view_plan, dim3(1), dim3(vv::kViewPlanWG), 0, st, a);
    return launched("view_plan");
}

int view_composite(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb <= 0) return 0;
    hipLaunchKernelGGL(vv::view_composite, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
    return launched("view_composite");
}

// ---- the scene forms: the same launches with the scene kernels and the scene's plan capacity ----
int scene_view_count(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb > 0) {
        hipLaunchKernelGGL(vv::scene_view_count, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
        if (int rc = launched("scene_view_count")) return rc;
    }
    hipLaunchKernelGGL(vv::view_scan, dim3(1), dim3(vv::kViewScanWG), 0, st, a);
    return launched("view_scan");
}

int scene_view_emit(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb > 0 && a.cap > 0) {
        hipLaunchKernelGGL(vv::scene_view_emit, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
        if (int rc = launched("scene_view_emit")) return rc;
    }
    hipError_t e = hipMemsetAsync(a.plan, 0xff, (size_t)kScenePlanCap * 4 * sizeof(int), st);     // no entry: object -1
    if (e != hipSuccess) return fail(-4, "hipMemsetAsync(scene view plan): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(vv::scene_view_plan, dim3(1), dim3(vv::kViewPlanWG), 0, st, a);
    return launched("scene_view_plan");
}

int scene_view_composite(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb <= 0) return 0;
    hipLaunchKernelGGL(vv::scene_view_composite, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
    return launched("scene_view_composite");
}

}  // namespace vl
