// TEST INFRASTRUCTURE: object bounds (bounds_kernels.h) on the CPU executor.  The launch sequences repeat vmap_amd/csrc/k_bounds.hip;
// workspace layouts and the automatic chunk count are the product's own (launch_geometry.h).
#include <cstring>

#include "bounds_kernels.h"
#include "launch_geometry.h"
#include "sim_runtime.h"

namespace {
struct Frames {
    const float* depth; const int* inst; const float* t_wc;
    int n_slots, width, height;
    float fx, fy, cx, cy;
};

vb::UnprojArgs unproject_args(const Frames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, void* workspace) {
    vb::UnprojArgs a;
    std::memset(&a, 0, sizeof(a));
    a.depth = f.depth; a.inst = f.inst; a.t_wc = f.t_wc; a.n_slots = f.n_slots; a.width = f.width; a.height = f.height;
    a.fx = f.fx; a.fy = f.fy; a.cx = f.cx; a.cy = f.cy;
    a.pairs = pairs; a.first_pair = first_pair; a.n_obj = n_obj; a.n_pairs = n_pairs; a.nb = vl::unproject_blocks(f.width, f.height);
    const vl::UnprojectLayout l = vl::unproject_layout(n_pairs, n_obj, f.width, f.height);
    a.blk = static_cast<long long*>(workspace);
    a.enc = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + l.off_enc);
    return a;
}

vb::ObbArgs obb_args(const float* points, const long long* po, int n_obj, const float* center) {
    vb::ObbArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = points; a.po = po; a.n_obj = n_obj; a.center = center;
    return a;
}
}  // namespace

// out: nb, off_enc, bytes
extern "C" void vmsim_unproject_layout(int n_pairs, int n_obj, int width, int height, long long* out) {
    const vl::UnprojectLayout l = vl::unproject_layout(n_pairs, n_obj, width, height);
    out[0] = vl::unproject_blocks(width, height); out[1] = (long long)l.off_enc; out[2] = (long long)l.bytes;
}

extern "C" int vmsim_unproject_count(const float* depth, const int* inst, const float* t_wc, int n_slots, int width, int height,
                                     const float* intr, const int* pairs, const int* first_pair, int n_obj, int n_pairs,
                                     long long* offsets, float* bounds, void* workspace) {
    const Frames f{depth, inst, t_wc, n_slots, width, height, intr[0], intr[1], intr[2], intr[3]};
    vb::UnprojArgs a = unproject_args(f, pairs, first_pair, n_obj, n_pairs, workspace);
    a.offsets = offsets; a.bounds = bounds;
    sim::launch((n_obj * 6 + vb::kBoundsWG - 1) / vb::kBoundsWG, vb::kBoundsWG, 0, [&] { vb::unproject_init(a); });
    if (n_pairs > 0) sim::launch3(a.nb, n_pairs, 1, vb::kBoundsWG, 0, [&] { vb::unproject_count(a); });
    sim::launch(1, vb::kScanWG, 0, [&] { vb::unproject_scan(a); });
    return 0;
}

extern "C" int vmsim_unproject_emit(const float* depth, const int* inst, const float* t_wc, int n_slots, int width, int height,
                                    const float* intr, const int* pairs, const int* first_pair, int n_obj, int n_pairs, float* points,
                                    long long n_points, void* workspace) {
    const Frames f{depth, inst, t_wc, n_slots, width, height, intr[0], intr[1], intr[2], intr[3]};
    vb::UnprojArgs a = unproject_args(f, pairs, first_pair, n_obj, n_pairs, workspace);
    a.out = points; a.cap = n_points;
    if (n_pairs > 0) sim::launch3(a.nb, n_pairs, 1, vb::kBoundsWG, 0, [&] { vb::unproject_emit(a); });
    return 0;
}

extern "C" int vmsim_obb_chunks(const long long* po, int n_obj, int K) { return vl::obb_chunks(po, n_obj, K); }

extern "C" int vmsim_obb_extents(const float* points, const long long* po, int n_obj, const float* center, const float* rotations,
                                 long long set_stride, int K, int chunks, float* lo, float* hi) {
    vb::ObbArgs a = obb_args(points, po, n_obj, center);
    a.rot = rotations; a.set_stride = set_stride; a.K = K; a.chunks = chunks;
    a.lo = reinterpret_cast<unsigned*>(lo); a.hi = reinterpret_cast<unsigned*>(hi);
    const unsigned flat = (unsigned)(((long long)n_obj * K * 3 + vb::kBoundsWG - 1) / vb::kBoundsWG);
    sim::launch(flat, vb::kBoundsWG, 0, [&] { vb::obb_init(a); });
    sim::launch3((K + vb::kObbBlock - 1) / vb::kObbBlock, chunks, n_obj, vb::kBoundsWG, 0, [&] { vb::obb_extents(a); });
    sim::launch(flat, vb::kBoundsWG, 0, [&] { vb::obb_decode(a); });
    return 0;
}

extern "C" int vmsim_cloud_moments(const float* points, const long long* po, int n_obj, const float* center, double* moments) {
    vb::ObbArgs a = obb_args(points, po, n_obj, center);
    a.moments = moments;
    sim::launch(n_obj, vb::kScanWG, 0, [&] { vb::cloud_moments(a); });
    return 0;
}

// the order-preserving encoding on its own: enc[i] = enc_f32(in[i]), dec[i] = dec_f32(enc[i]), one value per lane
extern "C" int vmsim_enc_dec(const float* in, long long n, unsigned* enc, float* dec) {
    sim::launch((unsigned)((n + 63) / 64), 64, 0, [&] {
        const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
        if (i < n) {
            enc[i] = vb::enc_f32(in[i]);
            dec[i] = vb::dec_f32(enc[i]);
        }
    });
    return 0;
}
