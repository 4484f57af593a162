// k_components.hip - mesh components (component_kernels.h): the labels of an indexed triangle mesh's connected components and the
// per-component statistics.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "component_kernels.h"
#include "launch.h"

namespace vl {

int components_label(const int* faces, long long n_faces, long long n_vertices, int* labels, long long* counts, void* workspace, hipStream_t st) {
    vcc::LabelArgs a;
    std::memset(&a, 0, sizeof(a));
    const ComponentLayout l = component_layout(n_vertices, n_faces);
    char* ws = static_cast<char*>(workspace);
    a.faces = faces; a.n_faces = n_faces; a.n_vertices = n_vertices; a.nvb = l.nvb;
    a.parent = reinterpret_cast<int*>(ws);
    a.dense = reinterpret_cast<int*>(ws + l.off_dense);
    a.vblk = reinterpret_cast<long long*>(ws + l.off_vblk);
    a.labels = labels; a.counts = counts;
    if (l.nvb > 0) {
        hipLaunchKernelGGL(vcc::comp_init, dim3((unsigned)l.nvb), dim3(vcc::kCompWG), 0, st, a);
        if (int rc = launched("comp_init")) return rc;
        if (l.nfb > 0) {
            hipLaunchKernelGGL(vcc::comp_hook, dim3((unsigned)l.nfb), dim3(vcc::kCompWG), 0, st, a);
            if (int rc = launched("comp_hook")) return rc;
        }
        hipLaunchKernelGGL(vcc::comp_flatten, dim3((unsigned)l.nvb), dim3(vcc::kCompWG), 0, st, a);
        if (int rc = launched("comp_flatten")) return rc;
    }
    hipLaunchKernelGGL(vcc::comp_scan, dim3(1), dim3(vcc::kCompScanWG), 0, st, a);       // no vertex: C = 0
    if (int rc = launched("comp_scan")) return rc;
    if (l.nvb > 0) {
        hipLaunchKernelGGL(vcc::comp_root_emit, dim3((unsigned)l.nvb), dim3(vcc::kCompWG), 0, st, a);
        if (int rc = launched("comp_root_emit")) return rc;
        hipLaunchKernelGGL(vcc::comp_relabel, dim3((unsigned)l.nvb), dim3(vcc::kCompWG), 0, st, a);
        if (int rc = launched("comp_relabel")) return rc;
    }
    return 0;
}

int components_stats(const float* vertices, const int* faces, long long n_faces, const int* labels, long long n_vertices, long long n_components,
                     int* comp_vertices, long long* comp_faces, long long* comp_area_q, hipStream_t st) {
    vcc::StatsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vertices = vertices; a.faces = faces; a.n_faces = n_faces; a.labels = labels; a.n_vertices = n_vertices; a.n_components = n_components;
    a.comp_vertices = comp_vertices;
    a.comp_faces = reinterpret_cast<unsigned long long*>(comp_faces);
    a.comp_area_q = reinterpret_cast<unsigned long long*>(comp_area_q);
    hipError_t e = hipMemsetAsync(comp_vertices, 0, (size_t)n_components * sizeof(int), st);
    if (e == hipSuccess) e = hipMemsetAsync(comp_faces, 0, (size_t)n_components * sizeof(long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(comp_area_q, 0, (size_t)n_components * sizeof(long long), st);
    if (e != hipSuccess) return fail(-4, "hipMemsetAsync(component statistics): %s", hipGetErrorString(e));
    if (n_faces > 0) {
        hipLaunchKernelGGL(vcc::comp_face_stats, dim3((unsigned)ceil_div(n_faces, vcc::kStatsWG)), dim3(vcc::kStatsWG), 0, st, a);
        if (int rc = launched("comp_face_stats")) return rc;
    }
    hipLaunchKernelGGL(vcc::comp_vertex_stats, dim3((unsigned)ceil_div(n_vertices, vcc::kStatsWG)), dim3(vcc::kStatsWG), 0, st, a);
    return launched("comp_vertex_stats");
}

}  // namespace vl
