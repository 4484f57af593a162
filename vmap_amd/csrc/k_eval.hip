// k_eval.hip - mesh evaluation (eval_kernels.h): nearest-neighbour distances over segmented point sets, area-weighted surface
// sampling, and cropping a mesh to an oriented box.  gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "eval_kernels.h"
#include "launch.h"

namespace vl {

static int grid_of(long long n) { return (int)((n + ve::kEvalWG - 1) / ve::kEvalWG); }

int nn_distance(const NnPlan& p, const float* queries, const long long* qo, const float* refs, const long long* ro, int n_sets,
                float* dist, int* index, void* workspace, hipStream_t st) {
    ve::NnArgs a;
    std::memset(&a, 0, sizeof(a));
    a.q = queries; a.r = refs; a.qo = qo; a.ro = ro; a.n_sets = n_sets; a.rchunk = p.rchunk;
    char* ws = static_cast<char*>(workspace);
    a.prefix = reinterpret_cast<long long*>(ws);
    a.keys = reinterpret_cast<unsigned long long*>(ws + nn_layout(p.n_queries, n_sets).off_keys);
    a.q_begin = p.q_begin; a.q_end = p.q_end; a.dist = dist; a.index = index;
    hipLaunchKernelGGL(ve::nn_plan, dim3(1), dim3(ve::kPlanWG), 0, st, a);
    if (int rc = launched("nn_plan")) return rc;
    hipLaunchKernelGGL(ve::nn_init, dim3(grid_of(p.q_end - p.q_begin)), dim3(ve::kEvalWG), 0, st, a);
    if (int rc = launched("nn_init")) return rc;
    hipLaunchKernelGGL(ve::nn_search, dim3((unsigned)p.items), dim3(ve::kNnWG), 0, st, a);
    if (int rc = launched("nn_search")) return rc;
    hipLaunchKernelGGL(ve::nn_finalize, dim3(grid_of(p.q_end - p.q_begin)), dim3(ve::kEvalWG), 0, st, a);
    return launched("nn_finalize");
}

int surface_sample(const float* vertices, long long n_vertices, const int* faces, const long long* fo, const long long* oo, int n_sets,
                   long long o_begin, long long o_end, unsigned long long seed, unsigned stream_id, int set_base, const double* u0,
                   const float* r, float* points, int* face_index, void* workspace, hipStream_t st) {
    ve::SurfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = vertices; a.n_vertices = n_vertices; a.f = faces; a.fo = fo; a.oo = oo; a.n_sets = n_sets;
    a.cdf = static_cast<double*>(workspace);
    a.o_begin = o_begin; a.o_end = o_end; a.out = points; a.face_index = face_index; a.u0 = u0; a.r = r;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32); a.stream = stream_id; a.set_base = set_base;
    hipLaunchKernelGGL(ve::surface_cdf, dim3(n_sets), dim3(ve::kCdfWG), 0, st, a);
    if (int rc = launched("surface_cdf")) return rc;
    hipLaunchKernelGGL(ve::surface_sample, dim3(grid_of(o_end - o_begin)), dim3(ve::kEvalWG), 0, st, a);
    return launched("surface_sample");
}

static ve::ClipArgs clip_args(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float box[15],
                              void* workspace) {
    ve::ClipArgs a;
    std::memset(&a, 0, sizeof(a));
    a.v = vertices; a.n_vertices = n_vertices; a.f = faces; a.n_faces = n_faces; a.nblk = grid_of(n_faces);
    for (int k = 0; k < 3; ++k) {
        a.c[k] = box[k];
        for (int i = 0; i < 3; ++i) a.ax[k][i] = box[3 + 3 * i + k];          // column k of the row-major R
        a.h[k] = 0.5f * box[12 + k];
    }
    a.blk = static_cast<long long*>(workspace);
    return a;
}

int clip_box_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float box[15], long long* count,
                   void* workspace, hipStream_t st) {
    ve::ClipArgs a = clip_args(vertices, n_vertices, faces, n_faces, box, workspace);
    a.count = count;
    if (a.nblk > 0) {
        hipLaunchKernelGGL(ve::clip_count, dim3(a.nblk), dim3(ve::kEvalWG), 0, st, a);
        if (int rc = launched("clip_count")) return rc;
    }
    hipLaunchKernelGGL(ve::clip_scan, dim3(1), dim3(ve::kPlanWG), 0, st, a);
    return launched("clip_scan");
}

int clip_box_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float box[15], float* triangles,
                  long long n_triangles, void* workspace, hipStream_t st) {
    ve::ClipArgs a = clip_args(vertices, n_vertices, faces, n_faces, box, workspace);
    a.out = triangles; a.cap = n_triangles;
    hipLaunchKernelGGL(ve::clip_emit, dim3(a.nblk), dim3(ve::kEvalWG), 0, st, a);
    return launched("clip_emit");
}

}  // namespace vl
