// k_cull.hip - visibility culling (cull_kernels.h): which points of a cloud any keyframe saw, and the compaction of a mesh by such a
// mask.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "cull_kernels.h"
#include "launch.h"

namespace vl {

int cull_mark(const vmapstep_cull_cfg& c, const float* points, long long n_points, const float* depth, const float* t_wc, const int* slots,
              int n_frames, unsigned char* seen, hipStream_t st) {
    vc::MarkArgs a;
    std::memset(&a, 0, sizeof(a));
    cr::Rules& r = a.rules;
    r.fx = c.fx; r.fy = c.fy; r.cx = c.cx; r.cy = c.cy;
    r.min_depth = c.min_depth; r.eps = c.occlusion_eps;
    r.width = c.width; r.height = c.height; r.margin = c.margin; r.use_depth = c.use_depth ? 1 : 0;
    a.points = points; a.n_points = n_points;
    a.depth = r.use_depth ? depth : nullptr;
    a.t_wc = t_wc; a.slots = slots; a.n_frames = n_frames; a.seen = seen;
    const long long tiles = ceil_div(n_points, vc::kCullTile), chunks = ceil_div(n_frames, vc::kFrameChunk);
    // frames are the slow grid dimension: the workgroups running at the same time work on the same few frames
    hipLaunchKernelGGL(vc::cull_mark, dim3((unsigned)tiles, (unsigned)(chunks < vc::kMaxChunkRows ? chunks : vc::kMaxChunkRows)), dim3(vc::kCullWG), 0,
                       st, a);
    return launched("cull_mark");
}

static vc::CompactArgs compact_args(const int* faces, long long n_faces, const unsigned char* seen, long long n_vertices, int min_seen,
                                    void* workspace) {
    vc::CompactArgs a;
    std::memset(&a, 0, sizeof(a));
    const CullLayout l = cull_layout(n_vertices, n_faces);
    char* ws = static_cast<char*>(workspace);
    a.faces = faces; a.n_faces = n_faces; a.seen = seen; a.n_vertices = n_vertices; a.min_seen = min_seen;
    a.nfb = l.nfb;
    a.nvb = n_faces > 0 ? l.nvb : 0;                       // no face, no referenced vertex: nothing to clear, count or scan
    a.used = reinterpret_cast<unsigned char*>(ws);
    a.newidx = reinterpret_cast<int*>(ws + l.off_newidx);
    a.fblk = reinterpret_cast<long long*>(ws + l.off_fblk);
    a.vblk = reinterpret_cast<long long*>(ws + l.off_vblk);
    return a;
}

int cull_faces_count(const int* faces, long long n_faces, const unsigned char* seen, long long n_vertices, int min_seen, long long* counts,
                     void* workspace, hipStream_t st) {
    vc::CompactArgs a = compact_args(faces, n_faces, seen, n_vertices, min_seen, workspace);
    a.counts = counts;
    if (a.nfb > 0) {
        hipLaunchKernelGGL(vc::cull_clear, dim3((unsigned)a.nvb), dim3(vc::kCullWG), 0, st, a);
        if (int rc = launched("cull_clear")) return rc;
        hipLaunchKernelGGL(vc::cull_face_count, dim3((unsigned)a.nfb), dim3(vc::kCullWG), 0, st, a);
        if (int rc = launched("cull_face_count")) return rc;
        hipLaunchKernelGGL(vc::cull_vertex_count, dim3((unsigned)a.nvb), dim3(vc::kCullWG), 0, st, a);
        if (int rc = launched("cull_vertex_count")) return rc;
    }
    hipLaunchKernelGGL(vc::cull_scan, dim3(1), dim3(vc::kCullScanWG), 0, st, a);
    return launched("cull_scan");
}

int cull_faces_emit(const int* faces, long long n_faces, const unsigned char* seen, long long n_vertices, int min_seen, int* kept_vertices,
                    long long n_kept_vertices, int* faces_out, long long n_kept_faces, void* workspace, hipStream_t st) {
    vc::CompactArgs a = compact_args(faces, n_faces, seen, n_vertices, min_seen, workspace);
    a.kept_vertices = kept_vertices; a.faces_out = faces_out;
    a.vertex_cap = n_kept_vertices; a.face_cap = n_kept_faces;
    hipLaunchKernelGGL(vc::cull_vertex_emit, dim3((unsigned)a.nvb), dim3(vc::kCullWG), 0, st, a);
    if (int rc = launched("cull_vertex_emit")) return rc;
    hipLaunchKernelGGL(vc::cull_face_emit, dim3((unsigned)a.nfb), dim3(vc::kCullWG), 0, st, a);
    return launched("cull_face_emit");
}

}  // namespace vl
