// k_raster.hip - the mesh rasteriser (raster_kernels.h): depth and face images of a mesh from poses, and the comparison of two depth
// stacks.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "raster_kernels.h"

namespace vl {

static vr::DrawArgs draw_args(const vmapstep_raster_cfg& c, const float* vertices, long long n_vertices, const int* faces, long long n_faces,
                              const float* t_wc, const int* slots, int n_views, unsigned long long* keys, void* workspace) {
    vr::DrawArgs a;
    std::memset(&a, 0, sizeof(a));
    rr::Camera& cam = a.cam;
    cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy;
    cam.min_depth = c.min_depth; cam.max_depth = c.max_depth;
    cam.width = c.width; cam.height = c.height;
    a.vertices = vertices; a.n_vertices = n_vertices; a.faces = faces; a.n_faces = n_faces;
    a.t_wc = t_wc; a.slots = slots; a.n_views = n_views;
    a.nfb = raster_layout(n_faces, n_views, 0).nfb;
    a.keys = keys;
    a.blk = static_cast<long long*>(workspace);
    return a;
}

int raster_count(const vmapstep_raster_cfg& c, const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* t_wc,
                 const int* slots, int n_views, unsigned long long* keys, int* dropped, long long* counts, void* workspace, hipStream_t st) {
    vr::DrawArgs a = draw_args(c, vertices, n_vertices, faces, n_faces, t_wc, slots, n_views, keys, workspace);
    a.dropped = dropped; a.counts = counts;
    const size_t key_bytes = (size_t)n_views * c.width * c.height * sizeof(unsigned long long);
    if (hipMemsetAsync(keys, 0xff, key_bytes, st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "raster_count: hipMemsetAsync(keys)");
    if (hipMemsetAsync(dropped, 0, (size_t)n_views * sizeof(int), st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "raster_count: hipMemsetAsync(dropped)");
    if (a.nfb > 0) {
        hipLaunchKernelGGL(vr::raster_setup, dim3((unsigned)a.nfb, (unsigned)n_views), dim3(vr::kRasterWG), 0, st, a);
        if (int rc = launched("raster_setup")) return rc;
    }
    hipLaunchKernelGGL(vr::raster_scan, dim3(1), dim3(vr::kRasterScanWG), 0, st, a);
    return launched("raster_scan");
}

int raster_draw(const vmapstep_raster_cfg& c, const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* t_wc,
                const int* slots, int n_views, unsigned long long* keys, long long n_large, long long n_pairs, void* large, long long large_cap,
                void* workspace, hipStream_t st) {
    vr::DrawArgs a = draw_args(c, vertices, n_vertices, faces, n_faces, t_wc, slots, n_views, keys, workspace);
    const RasterLayout l = raster_layout(n_faces, n_views, large_cap);
    a.first = static_cast<long long*>(large);
    a.recs = reinterpret_cast<vr::LargeRec*>(static_cast<char*>(large) + l.off_rec);
    a.large_cap = large_cap; a.n_large = n_large; a.n_pairs = n_pairs;
    // a record raster_emit does not write (counts that are not the count call's) stays all zero: no tile, raster_tiles draws nothing
    if (hipMemsetAsync(large, 0, l.large_bytes, st) != hipSuccess) return fail(VMAPSTEP_ERR_DEVICE, "raster_draw: hipMemsetAsync(large)");
    hipLaunchKernelGGL(vr::raster_emit, dim3((unsigned)a.nfb, (unsigned)n_views), dim3(vr::kRasterWG), 0, st, a);
    if (int rc = launched("raster_emit")) return rc;
    long long blocks = ceil_div(n_pairs, vr::kTilesPerWG);
    blocks = blocks > vr::kMaxTileBlocks ? vr::kMaxTileBlocks : blocks;
    hipLaunchKernelGGL(vr::raster_tiles, dim3((unsigned)blocks), dim3(vr::kRasterWG), 0, st, a);
    return launched("raster_tiles");
}

int raster_resolve(const unsigned long long* keys, long long n_pixels, float* depth, int* face, const int* face_labels, long long n_faces, int* label,
                   unsigned char* face_seen, hipStream_t st) {
    vr::ResolveArgs a;
    std::memset(&a, 0, sizeof(a));
    a.keys = keys; a.n_pixels = n_pixels; a.depth = depth; a.face = face;
    a.face_labels = face_labels; a.n_faces = n_faces; a.label = label; a.face_seen = face_seen;
    hipLaunchKernelGGL(vr::raster_resolve, dim3((unsigned)ceil_div(n_pixels, vr::kResolveWG)), dim3(vr::kResolveWG), 0, st, a);
    return launched("raster_resolve");
}

int depth_compare(const float* a_depth, const float* b_depth, int n_views, long long pixels, long long* out, hipStream_t st) {
    vr::CompareArgs a;
    std::memset(&a, 0, sizeof(a));
    a.a = a_depth; a.b = b_depth; a.pixels = pixels; a.out = reinterpret_cast<unsigned long long*>(out);
    if (hipMemsetAsync(out, 0, (size_t)n_views * vr::kCompareInts * sizeof(long long), st) != hipSuccess)
        return fail(VMAPSTEP_ERR_DEVICE, "depth_compare: hipMemsetAsync(out)");
    hipLaunchKernelGGL(vr::depth_compare, dim3((unsigned)ceil_div(pixels, vr::kCompareBlock), (unsigned)n_views), dim3(vr::kCompareWG), 0, st, a);
    return launched("depth_compare");
}

}  // namespace vl
