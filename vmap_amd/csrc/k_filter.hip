// k_filter.hip - the instance filter (filter_kernels.h): the statistics and status of every instance id of a decoded frame against the
// boxes registered so far, the voxel keys that join the ids' clouds, the label image, and the decoding of keys to points.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "filter_kernels.h"
#include "launch.h"

static_assert(VMAPSTEP_FILTER_MAX_CLASSES == fr::kMaxClasses, "background class list");
static_assert(VMAPSTEP_FILTER_ROW_INTS == fr::kRowInts && VMAPSTEP_FILTER_HEAD_INTS == fr::kHeadInts && VMAPSTEP_FILTER_BOX_FLOATS == fr::kBoxFloats,
              "row layouts");
static_assert(vf::kMaxIds == fr::kMaxIds && vf::kMaxRadius == fr::kMaxRadius, "limits");

namespace vl {

static vf::FilterArgs filter_args(const vmapstep_filter_cfg& c, const void* depth, const void* inst, const void* sem, const float* box_table,
                                  int* status, void* workspace) {
    vf::FilterArgs a;
    std::memset(&a, 0, sizeof(a));
    fr::Rules& r = a.rules;
    r.width = c.width; r.height = c.height;
    r.depth_scale = c.depth_scale; r.max_depth = c.max_depth;
    r.cam.fx = c.fx; r.cam.fy = c.fy; r.cam.cx = c.cx; r.cam.cy = c.cy;
    for (int k = 0; k < 12; ++k) r.cam.T[k] = c.t_wc[k];
    r.voxel = c.voxel_size;
    r.id_shift = c.id_shift; r.min_pixels = c.min_pixels; r.min_points = c.min_points; r.erode_radius = c.erode_radius; r.max_ids = c.max_ids;
    r.n_background = c.n_background;
    for (int k = 0; k < c.n_background; ++k) r.background[k] = c.background_classes[k];
    a.label_i32 = c.label_i32; a.depth_f32 = c.depth_f32;
    a.depth = depth; a.inst = inst; a.sem = sem; a.box_table = box_table; a.status = status;
    a.n_pix = (long long)c.width * c.height;
    a.n_blk = filter_pix_blocks(c.width, c.height);
    a.vec_ok = (reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(inst)) % 16 == 0;
    if (workspace) {
        const FilterLayout l = filter_layout(c.max_ids, c.width, c.height);
        char* ws = static_cast<char*>(workspace);
        a.overflow = reinterpret_cast<int*>(ws);
        a.table = reinterpret_cast<int*>(ws + l.off_table);
        a.flags = reinterpret_cast<unsigned char*>(ws + l.off_flags);
        a.blk = reinterpret_cast<int*>(ws + l.off_blk);
    }
    return a;
}

int filter_stats(const vmapstep_filter_cfg& c, const void* depth, const void* inst, const void* sem, const float* box_table, int* status,
                 int* rows_out, void* workspace, hipStream_t st) {
    vf::FilterArgs a = filter_args(c, depth, inst, sem, box_table, status, workspace);
    a.rows_out = rows_out;
    hipLaunchKernelGGL(vf::filter_init, dim3((unsigned)ceil_div((long long)vf::kReplicas * c.max_ids * vf::kTableInts, vf::kFilterWG)),
                       dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("filter_init")) return rc;
    hipLaunchKernelGGL(vf::filter_stats, dim3((unsigned)ceil_div(c.width, vf::kTileW), (unsigned)ceil_div(c.height, vf::kTileH)), dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("filter_stats")) return rc;
    hipLaunchKernelGGL(vf::filter_decide, dim3(1), dim3(vf::kDecideWG), 0, st, a);
    return launched("filter_decide");
}

int filter_emit(const vmapstep_filter_cfg& c, const void* depth, const void* inst, const int* status, unsigned long long* keys_out,
                int* rows_out, void* workspace, hipStream_t st) {
    vf::FilterArgs a = filter_args(c, depth, inst, nullptr, nullptr, const_cast<int*>(status), workspace);
    a.rows_out = rows_out; a.keys_out = keys_out;
    hipLaunchKernelGGL(vf::filter_count, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("filter_count")) return rc;
    hipLaunchKernelGGL(vf::filter_scan, dim3(1), dim3(vf::kDecideWG), 0, st, a);
    if (int rc = launched("filter_scan")) return rc;
    hipLaunchKernelGGL(vf::filter_emit, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    return launched("filter_emit");
}

int filter_write(const vmapstep_filter_cfg& c, const void* depth, const void* inst, const float* box_table, const int* status, int* labels_out,
                 hipStream_t st) {
    vf::FilterArgs a = filter_args(c, depth, inst, nullptr, box_table, const_cast<int*>(status), nullptr);
    a.labels_out = labels_out;
    a.vec_ok = a.vec_ok && reinterpret_cast<uintptr_t>(labels_out) % 16 == 0;
    hipLaunchKernelGGL(vf::filter_write, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    return launched("filter_write");
}

int voxel_points(const unsigned long long* keys, long long n_keys, const long long* offsets, int n_seg, float voxel, float* points, float* bounds,
                 hipStream_t st) {
    vf::VoxelArgs a{keys, n_keys, offsets, n_seg, voxel, points, bounds};
    hipLaunchKernelGGL(vf::voxel_points, dim3((unsigned)n_seg), dim3(vf::kFilterWG), 0, st, a);
    return launched("voxel_points");
}

}  // namespace vl
