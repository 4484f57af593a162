// k_icp.hip - the depth tracker (icp_kernels.h): the depth pyramid with its normal maps, one iteration's 29 integer sums, and the chain
// of (icp_reduce, icp_solve) launches of a whole frame-to-model alignment.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "icp_kernels.h"

static_assert(VMAPSTEP_ICP_MAX_LEVELS == icp::kMaxLevels && VMAPSTEP_ICP_MAX_LEVELS == vi::kMaxLevels, "levels");
static_assert(VMAPSTEP_ICP_SUMS == icp::kSums && VMAPSTEP_ICP_SUMS == vi::kSums && VMAPSTEP_ICP_LOG_COLS == icp::kLogCols, "row layouts");
static_assert(VMAPSTEP_ICP_MAX_PIXELS == icp::kMaxPixels && VMAPSTEP_ICP_STATE_BYTES == vi::kStateBytes, "limits");
static_assert(VMAPSTEP_ICP_MAX_ITERATIONS == vi::kMaxIterations, "limits");
static_assert(VMAPSTEP_ICP_OK == icp::OK && VMAPSTEP_ICP_DEGENERATE == icp::DEGENERATE && VMAPSTEP_ICP_SKIPPED == icp::SKIPPED, "statuses");
static_assert(vi::kSums * sizeof(unsigned long long) <= vi::kFlagOffset && vi::kFlagOffset + sizeof(int) <= vi::kStateBytes, "the state block");
static_assert(vi::kSums <= vi::kReduceWG && vi::kReduceWG % 64 == 0, "one lane per sum");

namespace vl {

static icp::Rules icp_rules(const vmapstep_icp_cfg& c) {
    icp::Rules r;
    r.min_depth = c.min_depth; r.max_depth = c.max_depth; r.band = c.band; r.dist_thresh = c.dist_thresh; r.cos_thresh = c.cos_thresh;
    return r;
}

static icp::Camera icp_camera(const vmapstep_icp_cfg& c, int level) {
    icp::Camera c0;
    c0.fx = c.fx; c0.fy = c.fy; c0.cx = c.cx; c0.cy = c.cy; c0.width = c.width; c0.height = c.height;
    return icp::level_camera(c0, level);
}

int icp_pyramid(const vmapstep_icp_cfg& c, const float* depth, void* maps, hipStream_t st) {
    const IcpLayout l = icp_layout(c.width, c.height, c.levels);
    float4* base = static_cast<float4*>(maps);
    for (int k = 0; k < c.levels; ++k) {
        vi::PyramidArgs a;
        std::memset(&a, 0, sizeof(a));
        a.rules = icp_rules(c);
        a.cam = icp_camera(c, k);
        a.first = k == 0;
        a.src = k == 0 ? depth : reinterpret_cast<const float*>(base + l.off[k - 1]) + 3;
        a.src_stride = k == 0 ? 1 : 4;
        a.src_w = k == 0 ? c.width : l.w[k - 1];
        a.src_h = k == 0 ? c.height : l.h[k - 1];
        a.out = base + l.off[k];
        hipLaunchKernelGGL(vi::icp_pyramid, dim3((unsigned)ceil_div(l.w[k], vi::kTileW), (unsigned)ceil_div(l.h[k], vi::kTileH)), dim3(vi::kPyramidWG), 0, st, a);
        if (int rc = launched("icp_pyramid")) return rc;
    }
    return VMAPSTEP_OK;
}

static vi::ReduceArgs reduce_args(const vmapstep_icp_cfg& c, const IcpLayout& l, const void* src_maps, const void* model_maps, int level) {
    vi::ReduceArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rules = icp_rules(c);
    a.cam = icp_camera(c, level);
    a.src = static_cast<const float4*>(src_maps) + l.off[level];
    a.model = static_cast<const float4*>(model_maps) + l.off[level];
    a.n_pix = l.w[level] * l.h[level];
    return a;
}

static unsigned reduce_grid(const vmapstep_icp_cfg& c, int n_pix) {
    const long long cap = c.grid_cap > 0 && c.grid_cap < vi::kReduceGrid ? c.grid_cap : vi::kReduceGrid;
    const long long need = ceil_div(n_pix, vi::kReduceWG);
    return (unsigned)(need < cap ? need : cap);
}

int icp_sums(const vmapstep_icp_cfg& c, const void* src_maps, const void* model_maps, int level, const double* t_sm, long long* sums, hipStream_t st) {
    const IcpLayout l = icp_layout(c.width, c.height, c.levels);
    vi::ReduceArgs a = reduce_args(c, l, src_maps, model_maps, level);
    a.pose = t_sm;
    a.sums = reinterpret_cast<unsigned long long*>(sums);
    if (hipMemsetAsync(sums, 0, vi::kSums * sizeof(long long), st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "icp_sums: hipMemsetAsync(sums)");
    hipLaunchKernelGGL(vi::icp_reduce, dim3(reduce_grid(c, a.n_pix)), dim3(vi::kReduceWG), 0, st, a);
    return launched("icp_reduce");
}

int icp_track(const vmapstep_icp_cfg& c, const void* src_maps, const void* model_maps, double* pose, double* log, long long* sums_log,
              double* pose_log, void* state, hipStream_t st) {
    const IcpLayout l = icp_layout(c.width, c.height, c.levels);
    unsigned long long* sums = static_cast<unsigned long long*>(state);
    int* done = reinterpret_cast<int*>(static_cast<char*>(state) + vi::kFlagOffset);
    if (hipMemsetAsync(state, 0, vi::kStateBytes, st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "icp_track: hipMemsetAsync(state)");
    int row = 0;
    for (int level = c.levels - 1; level >= 0; --level) {
        vi::ReduceArgs a = reduce_args(c, l, src_maps, model_maps, level);
        a.pose = pose; a.done = done; a.sums = sums;
        const unsigned grid = reduce_grid(c, a.n_pix);
        for (int it = 0; it < c.iterations[level]; ++it, ++row) {
            hipLaunchKernelGGL(vi::icp_reduce, dim3(grid), dim3(vi::kReduceWG), 0, st, a);
            if (int rc = launched("icp_reduce")) return rc;
            vi::SolveArgs s;
            std::memset(&s, 0, sizeof(s));
            s.p.damping = c.damping; s.p.pivot_rel = c.pivot_rel; s.p.eps = c.eps; s.p.min_inliers = c.min_inliers;
            s.sums = sums; s.pose = pose; s.done = done;
            s.log = log + (long long)row * icp::kLogCols;
            s.sums_log = sums_log + (long long)row * vi::kSums;
            s.pose_log = pose_log + (long long)row * 12;
            s.last_of_level = it == c.iterations[level] - 1;
            hipLaunchKernelGGL(vi::icp_solve, dim3(1), dim3(vi::kSolveWG), 0, st, s);
            if (int rc = launched("icp_solve")) return rc;
        }
    }
    return VMAPSTEP_OK;
}

}  // namespace vl
