// launch.h - host-side launchers of the kernel families, one translation unit per family so that hipcc compiles them side
// by side (build(): vmapstep.hip = the C ABI, k_f32.hip, k_s32.hip, k_ws.hip, k_ws8.hip, k_wp.hip, k_misc.hip, k_mesh.hip, k_eval.hip, k_bounds.hip, k_view.hip, k_ingest.hip, k_filter.hip, k_track.hip, k_cull.hip, k_components.hip, k_raster.hip, k_icp.hip, k_tsdf.hip, k_raycast.hip; no device code crosses
// a unit, so no relocatable device code is needed).  Every function only ENQUEUES on `st` and returns a vmapstep status.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include "launch_geometry.h"
#include "query_kernels.h"
#include "sample_kernels.h"
#include "step_kernels.h"
#include "view_args.h"

namespace vk { struct WsArgs; }
struct vmapstep_ingest_cfg;
struct vmapstep_filter_cfg;
struct vmapstep_track_cfg;
struct vmapstep_cull_cfg;
struct vmapstep_raster_cfg;
struct vmapstep_icp_cfg;
struct vmapstep_tsdf_cfg;
struct vmapstep_raycast_cfg;

namespace vl {

// vmapstep.hip
int fail(int code, const char* fmt, ...);                                        // sets vmapstep_last_error(), returns code
int ensure_dynamic_lds(const void* kernel, size_t bytes, const char* what);     // hipFuncSetAttribute once per (device, kernel)
int launched(const char* what);                                                  // hipGetLastError() -> status
// Measurement (vmapstep_profile_train_steps): while set on the calling thread, the dominant kernel's launch carries these two
// events - they take the dispatch's own begin / end timestamps (what a rocprofv3 kernel trace reports), not the stream's
struct DispatchEvents { hipEvent_t start, stop; };
extern thread_local const DispatchEvents* g_dispatch_events;
#define VL_LAUNCH_MAIN(kern, grid, block, lds, st, ...)                                                                     \
    do {                                                                                                                    \
        if (const vl::DispatchEvents* de_ = vl::g_dispatch_events)                                                          \
            hipExtLaunchKernelGGL(kern, grid, block, lds, st, de_->start, de_->stop, 0, __VA_ARGS__);                       \
        else                                                                                                                \
            hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);                                                    \
    } while (0)

// k_f32.hip: the exact-fp32 matrix-instruction kernels (step_main_h32, step_main_gen, step_main_wide<4>) and the
// width-generic prep / finalize kernels
int main_f32(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st);      // by a.hidden / a.wide
int prep_f32(const vk::StepArgs& a, int blocks, hipStream_t st);                 // step_prep: blocks = n_steps + pack blocks
int finalize_generic(const vk::FinalizeArgs& f, int grid, hipStream_t st);       // step_finalize
int finalize_h32(const vk::FinalizeArgs& f, const vk::FinalizeHot& h, int grid, hipStream_t st);

// k_s32.hip: hidden 32 on the bf16 matrix pipe with split operands
int main_s32(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st);
int prep_s32(const vk::StepArgs& a, int n_steps, hipStream_t st);
int finalize_s32(const vk::FinalizeArgs& f, const vk::FinalizeHot& h, int grid, hipStream_t st);

// k_ws.hip / k_wp.hip: hidden 64 / 128 on the bf16 matrix pipe (one wave / two waves per output block)
int main_ws(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st);
int main_wp(const vk::StepArgs& a, bool bwd, bool stamps, hipStream_t st);
int prep_ws(const vk::StepArgs& a, int n_steps, hipStream_t st);
int finalize_ws(const vk::FinalizeArgs& f, const vk::FinalizeHot& h, const int* tab_wt, hipStream_t st);
// k_ws8.hip: hidden 256 on the same scheme with eight waves (called through main_ws / prep_ws / finalize_ws)
int main_ws8(const vk::StepArgs& a, bool bwd, hipStream_t st);
int prep_ws8(const vk::WsArgs& ga, int n_steps, hipStream_t st);
int finalize_ws8(const vk::FinalizeArgs& f, const vk::FinalizeHot& h, const int* tab_wt, hipStream_t st);

// k_misc.hip: inference query and the frame sampler
int query_points(int hidden, const vk::StepArgs& pack, const vk::QueryArgs& q, long long n_points, hipStream_t st);
int sample_frame(const vs::SampleArgs& a, int n_obj, long long rays_per_object, hipStream_t st);   // a.obj_max != null: the split form (two launches)
// view rendering, the field pass of ONE group: the pack of the group's images (pack.hidden: step_prep_s32 at 32, step_prep wider), then
// field_query_seg_s32 / field_query_seg_gen<hidden / 32> over the group's `entries` plan entries.  `a` is the group's argument block
int view_field(const vk::StepArgs& pack, const vv::ViewArgs& a, long long entries, hipStream_t st);

// The mesh, evaluation and bounds families below take their block sizes, workspace layouts and launch plans from launch_geometry.h
// (vl::mesh_layout, nn_layout, nn_plan_host, surface_sample_bytes, clip_box_bytes, unproject_blocks, unproject_layout, obb_chunks).
// k_mesh.hip: marching cubes (mesh_kernels.h) and the dense grid Trainer.meshing queries.  The workspace of a [nx][ny][nz] volume:
// per-workgroup (vertices, faces) int64 pairs, then the first vertex id (int32) and the crossing-edge mask (uint8) of every point.
int mesh_grid_points(int nx, int ny, int nz, const float affine[12], float* points, hipStream_t st);
// valid: null = no mask; otherwise [n] bytes, non-zero = the point holds a value (cells with an invalid corner do not exist)
int mesh_count(const float* volume, const unsigned char* valid, int nx, int ny, int nz, float level, long long* counts, void* workspace,
               hipStream_t st);
// affine / ninv: null = index space; otherwise [A | b] rows and the inverse transpose of A (rows, for the normals)
// edge_ids: null, or [n_vertices] int32 = owning point * 3 + axis of every vertex
int mesh_emit(const float* volume, const unsigned char* valid, int nx, int ny, int nz, float level, const float* affine, const float* ninv,
              float* vertices, float* normals, int* faces, int* edge_ids, long long n_vertices, long long n_faces, void* workspace,
              hipStream_t st);

// k_eval.hip: mesh evaluation (eval_kernels.h).  Nearest neighbours: the workspace holds the per-set prefix of the work items
// (int64 [n_sets + 1]) and one packed (squared distance, index) key per query (uint64 [n_queries]).
int nn_distance(const NnPlan& p, const float* queries, const long long* qo, const float* refs, const long long* ro, int n_sets,
                float* dist, int* index, void* workspace, hipStream_t st);
// surface sampling: the workspace (surface_sample_bytes) is the float64 cumulative area of every face
int surface_sample(const float* vertices, long long n_vertices, const int* faces, const long long* fo, const long long* oo, int n_sets,
                   long long o_begin, long long o_end, unsigned long long seed, unsigned stream_id, int set_base, const double* u0,
                   const float* r, float* points, int* face_index, void* workspace, hipStream_t st);
// box clipping: the workspace (clip_box_bytes) is one int64 per block of ve::kEvalWG faces
int clip_box_count(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float box[15], long long* count,
                   void* workspace, hipStream_t st);
int clip_box_emit(const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float box[15], float* triangles,
                  long long n_triangles, void* workspace, hipStream_t st);

// k_bounds.hip: object bounds (bounds_kernels.h).  Unprojection: the workspace holds one int64 per (pair, vb::kPixBlock pixels) and the
// encoded coordinate extremes of every object (uint32 [n_obj][6]).
struct UnprojectFrames {
    const float* depth; const int* inst; const float* t_wc;
    int n_slots, width, height;
    float fx, fy, cx, cy;
};
int unproject_count(const UnprojectFrames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, long long* offsets,
                    float* bounds, void* workspace, hipStream_t st);
int unproject_emit(const UnprojectFrames& f, const int* pairs, const int* first_pair, int n_obj, int n_pairs, float* points,
                   long long n_points, void* workspace, hipStream_t st);
// chunks: point chunks per object (vl::obb_chunks picks it); the result does not depend on it (minimum and maximum are exact)
int obb_extents(const float* points, const long long* po, int n_obj, const float* center, const float* rotations, long long set_stride,
                int K, int chunks, float* lo, float* hi, hipStream_t st);
int cloud_moments(const float* points, const long long* po, int n_obj, const float* center, double* moments, hipStream_t st);


// k_view.hip: view rendering (view_kernels.h).  The workspace is vl::scene_layout's; ViewArgs carries its sections and the field groups.
int view_count(const vv::ViewArgs& a, hipStream_t st);                           // view_count, view_scan -> a.offsets
int view_emit(const vv::ViewArgs& a, hipStream_t st);                            // view_emit, view_plan (a.g_per from scene_plan_host)
int view_composite(const vv::ViewArgs& a, hipStream_t st);

// k_ingest.hip: frame ingest (ingest_kernels.h): ingest_init, ingest_stats, ingest_decide, ingest_write on `st`, nothing between them.
// The workspace is vl::ingest_layout's; rows_out holds 2 + max_ids * 8 int32.  inst / sem may be null (no labels / class 0 everywhere).
int ingest_frame(const vmapstep_ingest_cfg& cfg, const void* rgb, const void* depth, const void* inst, const void* sem, void* out_rgbx,
                 float* out_depth, int* out_inst, int* rows_out, void* workspace, hipStream_t st);

// k_filter.hip: the instance filter (filter_kernels.h).  The workspace is vl::filter_layout's; rows_out holds 4 + max_ids * 8 int32,
// status max_ids int32, box_table max_ids * 16 float32, keys_out width * height uint64.
// filter_init, filter_stats, filter_decide:
int filter_stats(const vmapstep_filter_cfg& cfg, const void* depth, const void* inst, const void* sem, const float* box_table, int* status,
                 int* rows_out, void* workspace, hipStream_t st);
// filter_count, filter_scan, filter_emit, on the workspace filter_stats left:
int filter_emit(const vmapstep_filter_cfg& cfg, const void* depth, const void* inst, const int* status, unsigned long long* keys_out,
                int* rows_out, void* workspace, hipStream_t st);
int filter_write(const vmapstep_filter_cfg& cfg, const void* depth, const void* inst, const float* box_table, const int* status, int* labels_out,
                 hipStream_t st);
int voxel_points(const unsigned long long* keys, long long n_keys, const long long* offsets, int n_seg, float voxel, float* points, float* bounds,
                 hipStream_t st);

// k_track.hip: the instance tracker (track_kernels.h).  The workspace is vl::track_layout's; meta holds det_class [max_det], pair_off
// [max_det + 1] and pair_inst [max_pairs] as int32; rows_out holds 4 + max_det * 9 + max_pairs int32, status and ident max_det int32
// each, box_table max_ids * 16 float32, keys_out width * height uint64.
// track_init, track_stats, track_decide:
int track_stats(const vmapstep_track_cfg& cfg, const void* depth, const void* det, const int* meta, const float* box_table, int* status,
                int* ident, int* rows_out, void* workspace, hipStream_t st);
// track_count, track_scan, track_emit, on the workspace track_stats left:
int track_emit(const vmapstep_track_cfg& cfg, const void* depth, const void* det, const float* box_table, const int* status, const int* ident,
               unsigned long long* keys_out, int* rows_out, void* workspace, hipStream_t st);
int track_write(const vmapstep_track_cfg& cfg, const void* depth, const void* det, const float* box_table, const int* status, const int* ident,
                int* labels_out, hipStream_t st);

// k_cull.hip: visibility culling (cull_kernels.h).  cull_mark only ever turns a 0 of `seen` into a 1.  The compaction's workspace is
// vl::cull_layout's: cull_faces_count = cull_clear, cull_face_count, cull_vertex_count, cull_scan -> counts {kept faces, kept vertices};
// cull_faces_emit = cull_vertex_emit, cull_face_emit on the workspace the count call left.
int cull_mark(const vmapstep_cull_cfg& cfg, const float* points, long long n_points, const float* depth, const float* t_wc, const int* slots,
              int n_frames, unsigned char* seen, hipStream_t st);
int cull_faces_count(const int* faces, long long n_faces, const unsigned char* seen, long long n_vertices, int min_seen, long long* counts,
                     void* workspace, hipStream_t st);
int cull_faces_emit(const int* faces, long long n_faces, const unsigned char* seen, long long n_vertices, int min_seen, int* kept_vertices,
                    long long n_kept_vertices, int* faces_out, long long n_kept_faces, void* workspace, hipStream_t st);

// k_components.hip: mesh components (component_kernels.h).  components_label = comp_init, comp_hook, comp_flatten, comp_scan ->
// counts {C}, comp_root_emit, comp_relabel on the workspace of vl::component_layout; components_stats zeroes the three outputs
// (memsets on the stream), then comp_face_stats and comp_vertex_stats.
int components_label(const int* faces, long long n_faces, long long n_vertices, int* labels, long long* counts, void* workspace, hipStream_t st);
int components_stats(const float* vertices, const int* faces, long long n_faces, const int* labels, long long n_vertices, long long n_components,
                     int* comp_vertices, long long* comp_faces, long long* comp_area_q, hipStream_t st);

// k_raster.hip: the mesh rasteriser (raster_kernels.h).  raster_count = keys to all ones, dropped to 0, raster_setup (small faces are
// drawn there), raster_scan -> counts {large faces, pairs} on the workspace of vl::raster_layout; raster_draw = the large-face buffer
// to 0, raster_emit, raster_tiles on the workspace the count call left; raster_resolve; depth_compare zeroes `out`, then adds.
int raster_count(const vmapstep_raster_cfg& cfg, const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* t_wc,
                 const int* slots, int n_views, unsigned long long* keys, int* dropped, long long* counts, void* workspace, hipStream_t st);
int raster_draw(const vmapstep_raster_cfg& cfg, const float* vertices, long long n_vertices, const int* faces, long long n_faces, const float* t_wc,
                const int* slots, int n_views, unsigned long long* keys, long long n_large, long long n_pairs, void* large, long long large_cap,
                void* workspace, hipStream_t st);
int raster_resolve(const unsigned long long* keys, long long n_pixels, float* depth, int* face, const int* face_labels, long long n_faces, int* label,
                   unsigned char* face_seen, hipStream_t st);
int depth_compare(const float* a, const float* b, int n_views, long long pixels, long long* out, hipStream_t st);

// k_icp.hip: the depth tracker (icp_kernels.h).  A maps buffer is vl::icp_layout's.  icp_pyramid = one icp_pyramid launch per level;
// icp_sums = sums to 0, one icp_reduce; icp_track = the state block to 0, then per level, coarse first, iterations[level] times
// (icp_reduce, icp_solve): log [n_iter][4] float64, sums_log [n_iter][29] int64, pose_log [n_iter][12] float64, pose [12] float64 in / out.
int icp_pyramid(const vmapstep_icp_cfg& cfg, const float* depth, void* maps, hipStream_t st);
int icp_sums(const vmapstep_icp_cfg& cfg, const void* src_maps, const void* model_maps, int level, const double* t_sm, long long* sums, hipStream_t st);
int icp_track(const vmapstep_icp_cfg& cfg, const void* src_maps, const void* model_maps, double* pose, double* log, long long* sums_log,
              double* pose_log, void* state, hipStream_t st);

// k_tsdf.hip: TSDF fusion (tsdf_kernels.h): one tsdf_integrate launch over all n_frames; color / rgbx / inst may be null (the C ABI has
// checked that what cfg makes the kernel read is there)
int tsdf_integrate(const vmapstep_tsdf_cfg& cfg, float* tsdf, float* weight, float* color, const float* depth, const unsigned char* rgbx,
                   const int* inst, const float* t_wc, const int* slots, int n_frames, hipStream_t st);

// k_raycast.hip: the TSDF ray cast (raycast_kernels.h).  tsdf_bricks = one launch, a workgroup per (a, b) column of bricks;
// tsdf_raycast = one launch per 65535 views; bricks null = the classes are not read; color / normal / color_out may be null
int tsdf_bricks(int nx, int ny, int nz, float min_weight, const float* tsdf, const float* weight, unsigned char* bricks, hipStream_t st);
int tsdf_raycast(const vmapstep_raycast_cfg& cfg, const float* tsdf, const float* weight, const float* color, const unsigned char* bricks, int n_bricks,
                 const float* views, int n_views, float* depth, unsigned char* status, float* normal, unsigned char* color_out, hipStream_t st);

}  // namespace vl
