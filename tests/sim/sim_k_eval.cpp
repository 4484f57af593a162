// TEST INFRASTRUCTURE: mesh evaluation (eval_kernels.h) on the CPU executor.  The launch sequences repeat vmap_amd/csrc/k_eval.hip; workspace
// layouts and the nearest-neighbour plan are the product's own (launch_geometry.h).
#include <cstring>

#include "eval_kernels.h"
#include "launch_geometry.h"
#include "sim_runtime.h"

namespace {
int grid_of(long long n) { return (int)((n + ve::kEvalWG - 1) / ve::kEvalWG); }

ve::ClipArgs clip_args(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* box, void* workspace) {
    ve::ClipArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = vertices; a.n_vertices = n_vertices; a.f = faces; a.n_faces = n_faces; a.nblk = grid_of(n_faces);
    for (int k = 0; k < 3; ++k) {
        a.c[k] = box[k];
        for (int i = 0; i < 3; ++i) a.ax[k][i] = box[3 + 3 * i + k];
        a.h[k] = 0.5f * box[12 + k];
    }
    a.blk = static_cast<long long*>(workspace);
    return a;
}
}  // namespace

// out: off_keys, bytes
extern "C" void vmsim_nn_layout(long long n_queries, int n_sets, long long* out) {
    const vl::NnLayout l = vl::nn_layout(n_queries, n_sets);
    out[0] = (long long)l.off_keys; out[1] = (long long)l.bytes;
}

// out: n_queries, q_begin, q_end, rchunk, items (vl::nn_plan_host); rchunk > 0 overrides the plan's refs per item (a multiple of
// ve::kNnTile) and the item count follows it by the plan's own formula
extern "C" int vmsim_nn_plan(const long long* qo, const long long* ro, int n_sets, long long n_queries, long long rchunk, long long* out) {
    vl::NnPlan p = vl::nn_plan_host(qo, ro, n_sets, n_queries);
    if (rchunk > 0) {
        if (rchunk % ve::kNnTile) return -1;
        p.rchunk = rchunk;
        p.items = 0;
        for (int s = 0; s < n_sets; ++s) {
            const long long nq = qo[s + 1] - qo[s], nr = ro[s + 1] - ro[s];
            if (nq > 0 && nr > 0) p.items += vl::ceil_div(nq, ve::kNnQB) * vl::ceil_div(nr, rchunk);
        }
    }
    out[0] = p.n_queries; out[1] = p.q_begin; out[2] = p.q_end; out[3] = p.rchunk; out[4] = p.items;
    return 0;
}

// plan: the five values of vmsim_nn_plan (q_begin / q_end may be narrowed by the caller)
extern "C" int vmsim_nn(const long long* plan, const float* queries, const long long* qo, const float* refs, const long long* ro, int n_sets,
                        float* dist, int* index, void* workspace) {
    ve::NnArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = queries; a.r = refs; a.qo = qo; a.ro = ro; a.n_sets = n_sets; a.rchunk = plan[3];
    char* ws = static_cast<char*>(workspace);
    a.prefix = reinterpret_cast<long long*>(ws);
    a.keys = reinterpret_cast<unsigned long long*>(ws + vl::nn_layout(plan[0], n_sets).off_keys);
    a.q_begin = plan[1]; a.q_end = plan[2]; a.dist = dist; a.index = index;
    sim::launch(1, ve::kPlanWG, 0, [&] { ve::nn_plan(a); });
    if (grid_of(a.q_end - a.q_begin) > 0) sim::launch(grid_of(a.q_end - a.q_begin), ve::kEvalWG, 0, [&] { ve::nn_init(a); });
    if (plan[4] > 0) sim::launch((unsigned)plan[4], ve::kNnWG, 0, [&] { ve::nn_search(a); });
    if (grid_of(a.q_end - a.q_begin) > 0) sim::launch(grid_of(a.q_end - a.q_begin), ve::kEvalWG, 0, [&] { ve::nn_finalize(a); });
    return 0;
}

extern "C" long long vmsim_surface_sample_bytes(long long n_faces) { return (long long)vl::surface_sample_bytes(n_faces); }

extern "C" int vmsim_surface_sample(const float* vertices, long long n_vertices, const int* faces, const long long* fo, const long long* oo,
                                    int n_sets, long long o_begin, long long o_end, unsigned long long seed, unsigned stream_id, int set_base,
                                    const double* u0, const float* r, float* points, int* face_index, void* workspace) {
    ve::SurfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = vertices; a.n_vertices = n_vertices; a.f = faces; a.fo = fo; a.oo = oo; a.n_sets = n_sets;
    a.cdf = static_cast<double*>(workspace);
    a.o_begin = o_begin; a.o_end = o_end; a.out = points; a.face_index = face_index; a.u0 = u0; a.r = r;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32); a.stream = stream_id; a.set_base = set_base;
    sim::launch(n_sets, ve::kCdfWG, 0, [&] { ve::surface_cdf(a); });
    if (grid_of(o_end - o_begin) > 0) sim::launch(grid_of(o_end - o_begin), ve::kEvalWG, 0, [&] { ve::surface_sample(a); });
    return 0;
}

extern "C" long long vmsim_clip_box_bytes(long long n_faces) { return (long long)vl::clip_box_bytes(n_faces); }

extern "C" int vmsim_clip_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* box,
                                long long* count, void* workspace) {
    ve::ClipArgs a = clip_args(vertices, n_vertices, faces, n_faces, box, workspace);
    a.count = count;
    if (a.nblk > 0) sim::launch(a.nblk, ve::kEvalWG, 0, [&] { ve::clip_count(a); });
    sim::launch(1, ve::kPlanWG, 0, [&] { ve::clip_scan(a); });
    return 0;
}

extern "C" int vmsim_clip_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* box,
                               float* triangles, long long n_triangles, void* workspace) {
    ve::ClipArgs a = clip_args(vertices, n_vertices, faces, n_faces, box, workspace);
    a.out = triangles; a.cap = n_triangles;
    if (a.nblk > 0) sim::launch(a.nblk, ve::kEvalWG, 0, [&] { ve::clip_emit(a); });
    return 0;
}
