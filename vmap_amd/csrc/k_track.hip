// k_track.hip - the instance tracker (track_kernels.h): the statistics of every detection row of a decoded frame, the number of its
// points inside the box of every known instance of its class, the decision made from those counts, the voxel keys that join the
// instances' clouds and the label image of persistent ids.  gfx950 only.
#include <cstdint>
#include <cstring>

#include "../../include/vmapstep.h"
#include "launch.h"
#include "track_kernels.h"

static_assert(VMAPSTEP_TRACK_ROW_INTS == tr::kRowInts && VMAPSTEP_TRACK_HEAD_INTS == tr::kHeadInts, "row layouts");
static_assert(VMAPSTEP_TRACK_MAX_DET == tr::kMaxDet && VMAPSTEP_TRACK_MAX_PAIRS == tr::kMaxPairs, "limits");
static_assert(vt::kMaxDet == tr::kMaxDet && vt::kMaxPairs == tr::kMaxPairs && vt::kStatInts == tr::kStatInts, "limits");
static_assert(VMAPSTEP_TRACK_PAIR_SLOTS == vt::kPairSlots, "the LDS pair table");
static_assert(vt::kPairSlots <= vf::kFilterWG && (vt::kPairSlots & (vt::kPairSlots - 1)) == 0, "one lane flushes one slot");

namespace vl {

static vt::TrackArgs track_args(const vmapstep_track_cfg& c, const void* depth, const void* det, const int* meta, const float* box_table,
                                int* status, int* ident, void* workspace) {
    vt::TrackArgs a;
    std::memset(&a, 0, sizeof(a));
    fr::Rules& r = a.rules.frame;
    r.width = c.width; r.height = c.height;
    r.depth_scale = c.depth_scale; r.max_depth = c.max_depth;
    r.cam.fx = c.fx; r.cam.fy = c.fy; r.cam.cx = c.cx; r.cam.cy = c.cy;
    for (int k = 0; k < 12; ++k) r.cam.T[k] = c.t_wc[k];
    r.voxel = c.voxel_size;
    r.id_shift = c.det_shift; r.min_pixels = c.min_pixels; r.min_points = c.min_points; r.erode_radius = c.erode_radius; r.max_ids = c.max_det;
    r.n_background = c.n_background;
    for (int k = 0; k < c.n_background; ++k) r.background[k] = c.background_classes[k];
    a.rules.max_ids = c.max_ids; a.rules.ratio_q = c.ratio_q; a.rules.next_id = c.next_id; a.rules.n_det = c.n_det;
    a.label_i32 = c.label_i32; a.depth_f32 = c.depth_f32;
    a.max_pairs = c.max_pairs; a.n_pairs = c.n_pairs;
    a.depth = depth; a.det = det; a.box_table = box_table; a.status = status; a.ident = ident;
    if (meta) {
        a.det_class = meta;
        a.pair_off = meta + c.max_det;
        a.pair_inst = meta + c.max_det + c.max_det + 1;
    }
    a.n_pix = (long long)c.width * c.height;
    a.n_blk = filter_pix_blocks(c.width, c.height);
    a.vec_ok = (reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(det)) % 16 == 0;
    if (workspace) {
        const TrackLayout l = track_layout(c.max_det, c.max_pairs, c.width, c.height);
        char* ws = static_cast<char*>(workspace);
        a.overflow = reinterpret_cast<int*>(ws);
        a.table = reinterpret_cast<int*>(ws + l.off_table);
        a.pairs = reinterpret_cast<int*>(ws + l.off_pairs);
        a.flags = reinterpret_cast<unsigned char*>(ws + l.off_flags);
        a.blk = reinterpret_cast<int*>(ws + l.off_blk);
    }
    return a;
}

int track_stats(const vmapstep_track_cfg& c, const void* depth, const void* det, const int* meta, const float* box_table, int* status,
                int* ident, int* rows_out, void* workspace, hipStream_t st) {
    vt::TrackArgs a = track_args(c, depth, det, meta, box_table, status, ident, workspace);
    a.rows_out = rows_out;
    const long long cells = (long long)vf::kReplicas * (c.max_det * vt::kStatInts > c.max_pairs ? c.max_det * vt::kStatInts : c.max_pairs);
    hipLaunchKernelGGL(vt::track_init, dim3((unsigned)ceil_div(cells, vf::kFilterWG)), dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("track_init")) return rc;
    hipLaunchKernelGGL(vt::track_stats, dim3((unsigned)ceil_div(c.width, vf::kTileW), (unsigned)ceil_div(c.height, vf::kTileH)), dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("track_stats")) return rc;
    hipLaunchKernelGGL(vt::track_decide, dim3(1), dim3(vf::kDecideWG), 0, st, a);
    return launched("track_decide");
}

int track_emit(const vmapstep_track_cfg& c, const void* depth, const void* det, const float* box_table, const int* status, const int* ident,
               unsigned long long* keys_out, int* rows_out, void* workspace, hipStream_t st) {
    vt::TrackArgs a = track_args(c, depth, det, nullptr, box_table, const_cast<int*>(status), const_cast<int*>(ident), workspace);
    a.rows_out = rows_out; a.keys_out = keys_out;
    hipLaunchKernelGGL(vt::track_count, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    if (int rc = launched("track_count")) return rc;
    hipLaunchKernelGGL(vt::track_scan, dim3(1), dim3(vf::kDecideWG), 0, st, a);
    if (int rc = launched("track_scan")) return rc;
    hipLaunchKernelGGL(vt::track_emit, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    return launched("track_emit");
}

int track_write(const vmapstep_track_cfg& c, const void* depth, const void* det, const float* box_table, const int* status, const int* ident,
                int* labels_out, hipStream_t st) {
    vt::TrackArgs a = track_args(c, depth, det, nullptr, box_table, const_cast<int*>(status), const_cast<int*>(ident), nullptr);
    a.labels_out = labels_out;
    a.vec_ok = a.vec_ok && reinterpret_cast<uintptr_t>(labels_out) % 16 == 0;
    hipLaunchKernelGGL(vt::track_write, dim3((unsigned)a.n_blk), dim3(vf::kFilterWG), 0, st, a);
    return launched("track_write");
}

}  // namespace vl
