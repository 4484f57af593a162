// k_ingest.hip - frame ingest (ingest_kernels.h): the statistics of every instance id of a decoded frame, the per-id decision with
// its enlarged 2-D box, and the transposing write of the frame into a FrameStore slot.  gfx950 only.
#include <cstring>

#include "../../include/vmapstep.h"
#include "ingest_kernels.h"
#include "launch.h"

static_assert(VMAPSTEP_INGEST_MAX_CLASSES == ir::kMaxClasses, "background class list");

namespace vl {

int ingest_frame(const vmapstep_ingest_cfg& c, const void* rgb, const void* depth, const void* inst, const void* sem, void* out_rgbx,
                 float* out_depth, int* out_inst, int* rows_out, void* workspace, hipStream_t st) {
    vi::IngestArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rules.width = c.width; a.rules.height = c.height;
    a.rules.half_scale = 0.5f * c.bbox_scale;                 // exact: float32(0.5 * scale)
    a.rules.min_box = c.min_box;
    a.rules.n_background = c.n_background;
    for (int k = 0; k < c.n_background; ++k) a.rules.background[k] = c.background_classes[k];
    a.rules.depth_scale = c.depth_scale; a.rules.max_depth = c.max_depth;
    a.max_ids = c.max_ids; a.label_i32 = c.label_i32; a.depth_f32 = c.depth_f32;
    a.rgb = static_cast<const unsigned char*>(rgb); a.depth = depth; a.inst = inst; a.sem = sem;
    a.out_rgbx = static_cast<unsigned*>(out_rgbx); a.out_depth = out_depth; a.out_inst = out_inst; a.rows_out = rows_out;
    const IngestLayout l = ingest_layout(c.max_ids);
    char* ws = static_cast<char*>(workspace);
    a.overflow = reinterpret_cast<int*>(ws);
    a.table = reinterpret_cast<int*>(ws + l.off_table);
    a.status = reinterpret_cast<int*>(ws + l.off_status);
    a.replicas = ingest_replicas(c.max_ids);
    a.n_pix = (long long)c.width * c.height;

    hipLaunchKernelGGL(vi::ingest_init, dim3((unsigned)ceil_div((long long)a.replicas * c.max_ids * vi::kTableInts, vi::kIngestWG)), dim3(vi::kIngestWG), 0, st, a);
    if (int rc = launched("ingest_init")) return rc;
    hipLaunchKernelGGL(vi::ingest_stats, dim3(ingest_stats_blocks(c.width, c.height)), dim3(vi::kIngestWG), 0, st, a);
    if (int rc = launched("ingest_stats")) return rc;
    hipLaunchKernelGGL(vi::ingest_decide, dim3(1), dim3(vi::kDecideWG), 0, st, a);
    if (int rc = launched("ingest_decide")) return rc;
    hipLaunchKernelGGL(vi::ingest_write, dim3((unsigned)ceil_div(c.width, vi::kTile), (unsigned)ceil_div(c.height, vi::kTile)), dim3(vi::kIngestWG), 0, st, a);
    return launched("ingest_write");
}

}  // namespace vl
