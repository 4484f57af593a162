// TEST INFRASTRUCTURE, and nothing else: a deliberately WRONG kernel, the self-test of the executor's wave-greedy schedules
// (tests/test_kernel_sim_geom.py).  It breaks scan_ops.h's barrier contract on purpose - two wg_exclusive_scan calls through ONE
// wsum with no barrier between them - and exists only to be run on the CPU executor: a schedule that lets no wave run ahead of
// another cannot see the mistake, the wave-greedy ones must.  Its corrected twin takes an array per scan, as mesh_count does.
#include "scan_ops.h"
#include "sim_runtime.h"

namespace {
constexpr int kHazardWG = 512;

void two_scans(bool one_wsum, const int* x, const int* y, int* ex, int* ey, int* totals) {
    __shared__ int wsum[2][kHazardWG / 64];
    const int t = threadIdx.x;
    int tx, ty;
    ex[t] = vscan::wg_exclusive_scan<kHazardWG>(x[t], wsum[0], tx);
    ey[t] = vscan::wg_exclusive_scan<kHazardWG>(y[t], one_wsum ? wsum[0] : wsum[1], ty);
    totals[2 * t] = tx;
    totals[2 * t + 1] = ty;
}
}  // namespace

extern "C" int vmsim_scan_hazard_lanes() { return kHazardWG; }

// one_wsum != 0: the wrong kernel
extern "C" int vmsim_scan_hazard(int one_wsum, const int* x, const int* y, int* ex, int* ey, int* totals) {
    sim::launch(1, kHazardWG, 0, [&] { two_scans(one_wsum != 0, x, y, ex, ey, totals); });
    return 0;
}
