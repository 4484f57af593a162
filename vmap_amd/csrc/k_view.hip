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
    hipError_t e = hipMemsetAsync(a.plan, 0xff, (size_t)a.plan_cap * 4 * sizeof(int), st);       // no entry: object -1
    if (e != hipSuccess) return fail(-4, "hipMemsetAsync(view plan): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(vv::view_plan, dim3(1), dim3(vv::kViewPlanWG), 0, st, a);
    return launched("view_plan");
}

int view_composite(const vv::ViewArgs& a, hipStream_t st) {
    if (a.nb <= 0) return 0;
    if (a.g_end[0] < a.n_obj) hipLaunchKernelGGL(vv::view_composite<true>, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);
    else hipLaunchKernelGGL(vv::view_composite<false>, dim3(a.nb), dim3(vv::kViewBlock), 0, st, a);     // one group: cam.samples is its S
    return launched("view_composite");
}

}  // namespace vl
