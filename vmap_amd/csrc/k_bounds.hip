// k_bounds.hip - object bounds (bounds_kernels.h): keyframe unprojection as count -> scan -> emit, the extents of a segmented cloud
// along candidate box frames, and the per-object moments behind the covariance frame.  gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "bounds_kernels.h"
#include "launch.h"

namespace vl {

static vb::UnprojArgs unproject_args(const UnprojectFrames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, void* workspace) {
    vb::UnprojArgs a;
    std::memset(&a, 0, sizeof(a));
    a.depth = f.depth; a.inst = f.inst; a.t_wc = f.t_wc; a.n_slots = f.n_slots; a.width = f.width; a.height = f.height;
    a.fx = f.fx; a.fy = f.fy; a.cx = f.cx; a.cy = f.cy;
    a.pairs = pairs; a.first_pair = first_pair; a.n_obj = n_obj; a.n_pairs = n_pairs; a.nb = unproject_blocks(f.width, f.height);
    const UnprojectLayout l = unproject_layout(n_pairs, n_obj, f.width, f.height);
    a.blk = static_cast<long long*>(workspace);
    a.enc = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + l.off_enc);
    return a;
}

int unproject_count(const UnprojectFrames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, long long* offsets,
                    float* bounds, void* workspace, hipStream_t st) {
    vb::UnprojArgs a = unproject_args(f, pairs, first_pair, n_obj, n_pairs, workspace);
    a.offsets = offsets; a.bounds = bounds;
    hipLaunchKernelGGL(vb::unproject_init, dim3((n_obj * 6 + vb::kBoundsWG - 1) / vb::kBoundsWG), dim3(vb::kBoundsWG), 0, st, a);
    if (int rc = launched("unproject_init")) return rc;
    if (n_pairs > 0) {
        hipLaunchKernelGGL(vb::unproject_count, dim3(a.nb, n_pairs), dim3(vb::kBoundsWG), 0, st, a);
        if (int rc = launched("unproject_count")) return rc;
    }
    hipLaunchKernelGGL(vb::unproject_scan, dim3(1), dim3(vb::kScanWG), 0, st, a);
    return launched("unproject_scan");
}

int unproject_emit(const UnprojectFrames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, float* points,
                   long long n_points, void* workspace, hipStream_t st) {
    vb::UnprojArgs a = unproject_args(f, pairs, first_pair, n_obj, n_pairs, workspace);
    a.out = points; a.cap = n_points;
    hipLaunchKernelGGL(vb::unproject_emit, dim3(a.nb, n_pairs), dim3(vb::kBoundsWG), 0, st, a);
    return launched("unproject_emit");
}

static vb::ObbArgs obb_args(const float* points, const long long* po, int n_obj, const float* center) {
    vb::ObbArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = points; a.po = po; a.n_obj = n_obj; a.center = center;
    return a;
}

int obb_extents(const float* points, const long long* po, int n_obj, const float* center, const float* rotations, long long set_stride,
                int K, int chunks, float* lo, float* hi, hipStream_t st) {
    vb::ObbArgs a = obb_args(points, po, n_obj, center);
    a.rot = rotations; a.set_stride = set_stride; a.K = K; a.chunks = chunks;
    a.lo = reinterpret_cast<unsigned*>(lo); a.hi = reinterpret_cast<unsigned*>(hi);
    const unsigned flat = (unsigned)(((long long)n_obj * K * 3 + vb::kBoundsWG - 1) / vb::kBoundsWG);
    hipLaunchKernelGGL(vb::obb_init, dim3(flat), dim3(vb::kBoundsWG), 0, st, a);
    if (int rc = launched("obb_init")) return rc;
    hipLaunchKernelGGL(vb::obb_extents, dim3((K + vb::kObbBlock - 1) / vb::kObbBlock, chunks, n_obj), dim3(vb::kBoundsWG), 0, st, a);
    if (int rc = launched("obb_extents")) return rc;
    hipLaunchKernelGGL(vb::obb_decode, dim3(flat), dim3(vb::kBoundsWG), 0, st, a);
    return launched("obb_decode");
}

int cloud_moments(const float* points, const long long* po, int n_obj, const float* center, double* moments, hipStream_t st) {
    vb::ObbArgs a = obb_args(points, po, n_obj, center);
    a.moments = moments;
    hipLaunchKernelGGL(vb::cloud_moments, dim3(n_obj), dim3(vb::kScanWG), 0, st, a);
    return launched("cloud_moments");
}

}  // namespace vl
