// launch_geometry.h - the launch geometry of the mesh, evaluation, bounds, view, ingest, filter, track, cull, component, raster and icp families: the constants that both the kernels
// (mesh_kernels.h, eval_kernels.h, bounds_kernels.h, view_kernels.h, ingest_kernels.h, filter_kernels.h, track_kernels.h, cull_kernels.h, component_kernels.h, raster_kernels.h, icp_kernels.h) and the host-side workspace layouts and launch plans (launch.h) are built on.
// constexpr values and host-side inline functions only, no device code and no HIP header: the C ABI unit sizes workspaces from them
// without compiling anyone's kernels, and the CPU executor of tests/sim lays out its buffers by the same definitions.
#pragma once
#include <cstddef>

namespace vm {
constexpr int kMeshWG = 256;               // points per workgroup of count / emit
constexpr int kScanWG = 1024;              // the single workgroup of mesh_scan
}  // namespace vm

namespace ve {
constexpr int kNnWG = 256;                 // lanes per nn_search workgroup
constexpr int kNnQ = 8;                    // queries per lane
constexpr int kNnQB = kNnWG * kNnQ;        // queries per work item
constexpr int kNnTile = 512;               // refs per LDS tile (float4 each: 8 KiB)
constexpr int kPlanWG = 1024;              // nn_plan, clip_scan
constexpr int kEvalWG = 256;               // the elementwise kernels, clip_count / clip_emit
}  // namespace ve

namespace vb {
constexpr int kBoundsWG = 256;             // unproject_count / _emit, obb_extents, the elementwise kernels
constexpr int kPixPer = 4;                 // consecutive pixels per lane of unproject_count / _emit
constexpr int kPixBlock = kBoundsWG * kPixPer;
constexpr int kScanWG = 1024;              // unproject_scan, cloud_moments
constexpr int kObbCand = 4;                // candidates per lane
constexpr int kObbBlock = kBoundsWG * kObbCand;   // candidates per block
constexpr int kObbTile = 512;              // points per LDS tile (float4 each: 8 KiB)
}  // namespace vb

namespace vv {
constexpr int kViewBlock = 64;             // pixels per block of view_count / _emit / _composite: one wave, one lane per pixel
constexpr int kViewScanWG = 1024;          // view_scan
constexpr int kViewPlanWG = 256;           // view_plan: one lane per object (n_obj <= kViewMaxObj)
constexpr int kViewMaxObj = 256;
constexpr int kViewMaxHits = 16;           // VMAPSTEP_VIEW_MAX_HITS
constexpr int kViewMaxSamples = 64;
constexpr int kViewChunk = 128;            // points per chunk of field_query_seg_s32 (four waves x 32-point tiles)
constexpr int kViewImgBytes = 81920;       // one object's split image (vk::Img32s::BYTES; asserted where both are visible)
constexpr int kViewMaxGroups = 4;          // VMAPSTEP_VIEW_MAX_GROUPS: field groups of a scene view
}  // namespace vv

namespace vi {
constexpr int kIngestWG = 256;             // ingest_init, ingest_stats, ingest_write
constexpr int kStatsPer = 8;               // consecutive rounds of kIngestWG pixels per ingest_stats workgroup
constexpr int kStatsPix = kIngestWG * kStatsPer;
constexpr int kSlots = 64;                 // ids the LDS table of one ingest_stats workgroup holds (a power of two)
constexpr int kProbes = 4;                 // slots an id tries before it goes to the global table directly
constexpr int kTableInts = 8;              // a row of the global table: count, u min, u max, v min, v max, class min, class max, unused
constexpr int kReplicas = 8;               // copies of the global table (workgroup b adds to copy b % kReplicas; ingest_decide merges them)
constexpr int kReplicaIds = 4096;          // ... while max_ids <= this (1 MiB of tables); one copy beyond
constexpr int kDecideWG = 1024;            // the single workgroup of ingest_decide
constexpr int kTile = 64;                  // ingest_write transposes kTile x kTile pixels per workgroup
constexpr int kMaxIds = 65537;             // every uint16 label and -1
constexpr int kMaxSide = 4095;             // the sampler's own limit on width and height
}  // namespace vi

namespace vf {
constexpr int kFilterWG = 256;             // every filter kernel but filter_decide and filter_scan
constexpr int kTileW = 64;                 // filter_stats: a workgroup owns kTileW x kTileH pixels (a wave: 64 columns of one row)
constexpr int kTileH = 16;
constexpr int kMaxRadius = 8;              // erode_radius <= this: the halo of the LDS tile
constexpr int kHaloW = kTileW + 2 * kMaxRadius;
constexpr int kHaloH = kTileH + 2 * kMaxRadius;
constexpr int kSlots = 64;                 // ids the LDS table of one filter_stats workgroup holds (a power of two)
constexpr int kProbes = 4;
constexpr int kTableInts = 8;              // a row of the global table: pixels, class min, class max, valid, inside, eroded, eroded_valid, unused
constexpr int kReplicas = 8;               // copies of the global table, as vi::kReplicas
constexpr int kDecideWG = 1024;            // the single workgroup of filter_decide and of filter_scan
constexpr int kPixPer = 4;                 // consecutive pixels per lane of filter_count / _emit / _write
constexpr int kPixBlock = kFilterWG * kPixPer;
constexpr int kMaxIds = 32767;
constexpr int kMaxSide = 4095;
}  // namespace vf

namespace vt {                             // the instance tracker: the tile, block and replica geometry is vf's
constexpr int kPairSlots = 64;             // (detection, candidate) pairs the LDS table of one track_stats workgroup holds (a power of two)
constexpr int kPairProbes = 4;
constexpr int kStatInts = 4;               // a row of the global table: pixels, valid, eroded, eroded_valid
constexpr int kMaxDet = 4096;
constexpr int kMaxPairs = 65536;
}  // namespace vt

namespace vc {
constexpr int kCullWG = 256;               // every cull kernel but cull_scan; faces / vertices per block of the compaction
constexpr int kPointsPer = 4;              // points per lane of cull_mark, kCullWG apart (a wave's 64 points are consecutive)
constexpr int kCullTile = kCullWG * kPointsPer;   // points per workgroup of cull_mark
constexpr int kFrameChunk = 32;            // frames whose poses one cull_mark workgroup stages in LDS at a time
constexpr int kMaxChunkRows = 65535;       // grid rows of cull_mark (a row takes every kMaxChunkRows-th chunk beyond that)
constexpr int kCullScanWG = 256;           // the single workgroup of cull_scan
}  // namespace vc

namespace vcc {
constexpr int kCompWG = 256;               // comp_init / _hook / _flatten / _root_emit / _relabel; vertices per block of the root numbering
constexpr int kCompScanWG = 256;           // the single workgroup of comp_scan
constexpr int kStatsWG = 1024;             // comp_face_stats / comp_vertex_stats: sixteen waves share one LDS table before the global atomics
constexpr int kStatsSlots = 64;            // rows of that table, keyed by component % kStatsSlots (a second component on a row goes straight to memory)
}  // namespace vcc

namespace vr {
constexpr int kRasterWG = 256;             // raster_setup / _emit: (view, face) pairs per block, one view per block row; raster_tiles: four waves
constexpr int kRasterScanWG = 1024;        // the single workgroup of raster_scan
constexpr int kScanPer = 8;                // consecutive block totals per lane of raster_scan: 8192 blocks per round
constexpr int kTilesPerWG = kRasterWG / 64;        // (view, face, tile) pairs per raster_tiles workgroup per round: one wave each
constexpr long long kMaxTileBlocks = 1ll << 20;    // grid of raster_tiles: beyond 4 M pairs a wave takes every (grid x 4)-th pair
constexpr int kLargeRecInts = 16;          // one large-face record: 64 bytes
constexpr int kResolveWG = 256;            // raster_resolve: one pixel per lane
constexpr int kCompareWG = 256;            // depth_compare
constexpr int kComparePer = 4;             // pixels per lane of depth_compare, kCompareWG apart
constexpr int kCompareBlock = kCompareWG * kComparePer;
constexpr int kCompareInts = 4;            // a view's row: n_both, n_a_only, n_b_only, sum_q
}  // namespace vr

namespace vi {                             // the depth tracker (icp_kernels.h)
constexpr int kMaxLevels = 4;
constexpr int kTileW = 8;                  // icp_pyramid: a workgroup's tile of the output level, one pixel per lane; h is the fast axis
constexpr int kTileH = 32;
constexpr int kPyramidWG = kTileW * kTileH;
constexpr int kReduceWG = 256;             // icp_reduce: four waves
constexpr int kReduceGrid = 256;           // its grid at most: one workgroup per compute unit, whatever the image (measured: profiles/icp_bench.json)
constexpr int kSolveWG = 64;               // icp_solve: one wave
constexpr int kSums = 29;
constexpr int kMaxIterations = 64;         // per level
constexpr int kStateBytes = 512;           // the state block: the 29 sums (uint64) at 0, the level's finished flag (int32) at kFlagOffset
constexpr int kFlagOffset = 256;
}  // namespace vi

namespace vtsdf {                          // TSDF fusion (tsdf_kernels.h)
constexpr int kTsdfWG = 256;               // tsdf_integrate: four waves
constexpr int kVoxelsPer = 4;              // voxels per lane, kTsdfWG apart (a wave's 64 voxels are consecutive along k)
constexpr int kTsdfTile = kTsdfWG * kVoxelsPer;   // voxels per workgroup
constexpr int kTsdfChunk = 32;             // frames whose poses and image offsets a workgroup stages in LDS at a time
}  // namespace vtsdf

namespace vray {                           // the TSDF ray cast (raycast_kernels.h)
constexpr int kBricksWG = 256;             // tsdf_bricks: one workgroup per (a, b) column of bricks, a lane per k; four waves
constexpr int kRaycastWG = 256;            // tsdf_raycast: four waves, each an 8 x 8 pixel tile (h fast)
constexpr int kTile = 8;
constexpr int kTilesPerWG = kRaycastWG / 64;
constexpr int kMaxViewsPerLaunch = 65535;  // views ride on grid.y; more views = more launches (a pixel's result does not depend on it)
#ifdef VMAPSTEP_AB
constexpr int kClassLdsBudget = 16;        // the measurement build: every test volume's class table misses it and is read from global memory
#else
constexpr int kClassLdsBudget = 32768;     // bytes of class table a workgroup stages in LDS: a 256^3 volume's 32^3 bricks just fit
#endif
}  // namespace vray

// ---- workspace layouts and launch plans (namespace vl: what launch.h's launchers and the C ABI build on) ----
namespace vl {

inline size_t ws_up(size_t x) { return (x + 255) / 256 * 256; }       // workspace sections start 256-byte aligned
inline long long ceil_div(long long x, long long d) { return (x + d - 1) / d; }

// Marching cubes.  The workspace of a [nx][ny][nz] volume: per-workgroup (vertices, faces) int64 pairs, then the first vertex id
// (int32) and the crossing-edge mask (uint8) of every point.
struct MeshLayout {
    long long n; int nblk; size_t off_firstv, off_emask, bytes;
};
inline MeshLayout mesh_layout(int nx, int ny, int nz) {
    MeshLayout l;
    l.n = (long long)nx * ny * nz;
    l.nblk = (int)ceil_div(l.n, vm::kMeshWG);
    l.off_firstv = ws_up((size_t)l.nblk * 2 * sizeof(long long));
    l.off_emask = l.off_firstv + ws_up((size_t)l.n * sizeof(int));
    l.bytes = l.off_emask + ws_up((size_t)l.n);
    return l;
}

// Nearest neighbours: the workspace holds the per-set prefix of the work items (int64 [n_sets + 1]) and one packed (squared
// distance, index) key per query (uint64 [n_queries]).
struct NnLayout {
    size_t off_keys, bytes;
};
inline NnLayout nn_layout(long long n_queries, int n_sets) {
    NnLayout l;
    l.off_keys = ws_up((size_t)(n_sets + 1) * sizeof(long long));
    l.bytes = l.off_keys + ws_up((size_t)n_queries * sizeof(unsigned long long));
    return l;
}
// The launch plan from the host copies of the offsets: refs per work item (a multiple of the ref tile, ve::kNnTile) chosen so
// that about kNnItemsTarget items exist (8 per CU), and the item count nn_plan computes on the device by the same formula.
struct NnPlan {
    long long n_queries, q_begin, q_end, rchunk, items;
};
constexpr long long kNnItemsTarget = 2048;
inline NnPlan nn_plan_host(const long long* qo, const long long* ro, int n_sets, long long n_queries) {
    constexpr long long qb = ve::kNnQB, tile = ve::kNnTile;
    NnPlan p;
    p.n_queries = n_queries; p.q_begin = qo[0]; p.q_end = qo[n_sets];
    long long work = 0;                                   // sum over sets of (query blocks x refs)
    for (int s = 0; s < n_sets; ++s) {
        const long long nq = qo[s + 1] - qo[s], nr = ro[s + 1] - ro[s];
        if (nq > 0) work += ceil_div(nq, qb) * nr;
    }
    long long rc = ceil_div(work, kNnItemsTarget);
    rc = rc < 2 * tile ? 2 * tile : rc;
    rc = ceil_div(rc, tile) * tile;
    p.rchunk = rc;
    p.items = 0;
    for (int s = 0; s < n_sets; ++s) {
        const long long nq = qo[s + 1] - qo[s], nr = ro[s + 1] - ro[s];
        if (nq > 0 && nr > 0) p.items += ceil_div(nq, qb) * ceil_div(nr, rc);
    }
    return p;
}

// surface sampling: the workspace is the float64 cumulative area of every face
inline size_t surface_sample_bytes(long long n_faces) { return ws_up((size_t)n_faces * sizeof(double)); }
// box clipping: the workspace is one int64 per block of ve::kEvalWG faces (triangles per block, then their exclusive prefix)
inline size_t clip_box_bytes(long long n_faces) { return ws_up((size_t)ceil_div(n_faces, ve::kEvalWG) * sizeof(long long)) + 256; }

// Unprojection: the workspace holds one int64 per (pair, vb::kPixBlock pixels) and the encoded coordinate extremes of every object
// (uint32 [n_obj][6]).
inline int unproject_blocks(int width, int height) { return (int)ceil_div((long long)width * height, vb::kPixBlock); }
struct UnprojectLayout {
    size_t off_enc, bytes;
};
inline UnprojectLayout unproject_layout(int n_pairs, int n_obj, int width, int height) {
    UnprojectLayout l;
    l.off_enc = ws_up((size_t)n_pairs * unproject_blocks(width, height) * sizeof(long long)) + 256;
    l.bytes = l.off_enc + ws_up((size_t)n_obj * 6 * sizeof(unsigned));
    return l;
}

// The automatic launch geometry of obb_extents: point chunks per object so that about kObbBlocksTarget workgroups exist (8 per CU),
// never more than the largest object has tiles of vb::kObbTile points.  The result does not depend on it (minimum and maximum are exact).
constexpr long long kObbBlocksTarget = 2048;
inline int obb_chunks(const long long* po, int n_obj, int K) {
    long long most = 0;
    for (int o = 0; o < n_obj; ++o) most = po[o + 1] - po[o] > most ? po[o + 1] - po[o] : most;
    const long long tiles = ceil_div(most, vb::kObbTile), per_chunk = ceil_div(K, vb::kObbBlock) * n_obj;
    long long c = ceil_div(kObbBlocksTarget, per_chunk);
    c = c > tiles ? tiles : c;
    return (int)(c < 1 ? 1 : c > 65535 ? 65535 : c);
}

// View rendering: up to vv::kViewMaxGroups field groups, each with its own hidden width and samples per hit, composited into one image
// (a view of one group is the plain case).  Objects are numbered through the groups in order.  The workspace of a call over the pixels
// [pix_begin, pix_end): group after group the parameter images of its objects in the layout its field kernel reads (hidden 32:
// vv::kViewImgBytes split images, packed by step_prep_s32; wider: view_wide_image_floats float32 images, what vk::gen_layout(hidden).imgp
// is - asserted in query_kernels.h), then one int64 per (object, block of vv::kViewBlock pixels) - the hits of the block, then (after
// view_scan) their exclusive prefix in (object, block) order - and the launch plan of the field kernels, `plan_cap` entries.
inline int view_blocks(long long pix_begin, long long pix_end) { return (int)ceil_div(pix_end - pix_begin, vv::kViewBlock); }
struct SceneGroup {
    int hidden, n_obj, samples;
};
constexpr long long view_wide_image_floats(int H) { return (4ll * H * H + 253ll * H + 72 + 1023) / 1024 * 1024; }
inline size_t view_group_image_bytes(int hidden) {
    return hidden == 32 ? (size_t)vv::kViewImgBytes : (size_t)view_wide_image_floats(hidden) * sizeof(float);
}
// Plan entries per group.  field_query_seg_s32: two workgroups per compute unit (2 x 80 KiB of LDS).  field_query_seg_gen is
// __launch_bounds__(kWG, 1) and from hidden 160 holds NB x 16 KiB of LDS: ONE workgroup is resident per compute unit, so 256 entries
// would fill the chip exactly once and any excess entry (every object rounds up once) would cost a whole second round.  Eight entries
// per compute unit (as kNnItemsTarget, kObbBlocksTarget) bound that tail by 1/8 of a compute unit's share; an entry has no set-up to
// amortise (the weights are streamed from L2, nothing is staged per workgroup).
constexpr long long kViewWgTarget = 512;
constexpr long long kViewWideWgTarget = 2048;
inline long long view_group_target(int hidden) { return hidden == 32 ? kViewWgTarget : kViewWideWgTarget; }
// entries the plan of any scene can hold (every object rounds up once); the single-group hidden-32 entry points of the C ABI keep
// their documented kViewWgTarget + vv::kViewMaxObj, so the capacity is a value of the layout
constexpr long long kScenePlanCap = vv::kViewMaxGroups * kViewWideWgTarget + vv::kViewMaxObj;
struct SceneLayout {
    size_t off_img[vv::kViewMaxGroups], off_blk, off_plan, bytes;
    int n_obj, plan_cap;                                                    // objects of all groups; plan entries
};
inline SceneLayout scene_layout(const SceneGroup* g, int n_groups, long long pix_begin, long long pix_end, int plan_cap) {
    SceneLayout l{};
    size_t at = 0;
    for (int i = 0; i < n_groups; ++i) {
        l.off_img[i] = at;
        at += ws_up((size_t)g[i].n_obj * view_group_image_bytes(g[i].hidden));
        l.n_obj += g[i].n_obj;
    }
    l.off_blk = at;
    l.off_plan = l.off_blk + ws_up((size_t)l.n_obj * view_blocks(pix_begin, pix_end) * sizeof(long long));
    l.plan_cap = plan_cap;
    l.bytes = l.off_plan + ws_up((size_t)plan_cap * 4 * sizeof(int));
    return l;
}
// The launch plan of one group's field kernel from the host copy of its pair offsets: one entry (object, first chunk, end chunk) per
// workgroup, chunks of vv::kViewChunk points, `per` chunks per workgroup chosen so that about `target` workgroups exist; view_plan
// writes the entries on the device by the same formula.  The output does not depend on the plan (a point's value depends on the point
// alone).
struct ViewPlan {
    long long per, entries;
};
inline ViewPlan view_plan_host_target(const long long* offsets, int n_obj, int samples, long long target) {
    long long chunks = 0;
    for (int k = 0; k < n_obj; ++k) chunks += ceil_div((offsets[k + 1] - offsets[k]) * samples, vv::kViewChunk);
    ViewPlan p;
    p.per = ceil_div(chunks, target);
    p.per = p.per < 1 ? 1 : p.per;
    p.entries = 0;
    for (int k = 0; k < n_obj; ++k) p.entries += ceil_div(ceil_div((offsets[k + 1] - offsets[k]) * samples, vv::kViewChunk), p.per);
    return p;
}
// The launch plan of a view: view_plan_host_target per group (its own sample count and workgroup target).  The entries of a group are
// contiguous: view_plan scans them in object order.  `shift`: the groups' sample sections lie one after the other, inside a group
// pair after pair, so sample s of pair pr (a global pair index) of group g is element pr * samples_g + shift[g] + s of sample_occ.
// `samples`: all groups.
struct ScenePlan {
    long long per[vv::kViewMaxGroups], entries[vv::kViewMaxGroups], first[vv::kViewMaxGroups], shift[vv::kViewMaxGroups], samples;
};
inline ScenePlan scene_plan_host(const long long* offsets, const SceneGroup* g, int n_groups) {
    ScenePlan p{};
    int k0 = 0;
    long long first = 0;
    for (int i = 0; i < n_groups; ++i) {
        const ViewPlan v = view_plan_host_target(offsets + k0, g[i].n_obj, g[i].samples, view_group_target(g[i].hidden));
        p.per[i] = v.per; p.entries[i] = v.entries; p.first[i] = first;
        p.shift[i] = p.samples - offsets[k0] * g[i].samples;
        p.samples += (offsets[k0 + g[i].n_obj] - offsets[k0]) * g[i].samples;
        first += v.entries;
        k0 += g[i].n_obj;
    }
    return p;
}

// Frame ingest.  The workspace: the overflow word (pixels whose id has no table row), the statistics of every id
// (int32 [replicas][max_ids][vi::kTableInts], row = id + 1) and the status of every id (int32 [max_ids]) that ingest_write relabels
// by.  The table is kept in several copies so that the workgroups' atomics on the rows of the large instances (the wall, the floor:
// every workgroup meets them) spread over several addresses; the result does not depend on the number of copies.
inline int ingest_replicas(int max_ids) { return max_ids <= vi::kReplicaIds ? vi::kReplicas : 1; }
struct IngestLayout {
    size_t off_table, off_status, bytes;
};
inline IngestLayout ingest_layout(int max_ids) {
    IngestLayout l;
    l.off_table = 256;
    l.off_status = l.off_table + ws_up((size_t)ingest_replicas(max_ids) * max_ids * vi::kTableInts * sizeof(int));
    l.bytes = l.off_status + ws_up((size_t)max_ids * sizeof(int));
    return l;
}
inline int ingest_stats_blocks(int width, int height) { return (int)ceil_div((long long)width * height, vi::kStatsPix); }

// Instance filter.  The workspace: the overflow word, the statistics of every id (int32 [vf::kReplicas][max_ids][vf::kTableInts], row =
// shifted id), one byte of flags per pixel (valid, inside, eroded: what filter_stats found and filter_emit selects by) and per block
// of vf::kPixBlock pixels of filter_count an (emitted, out of grid) pair of int32, the first of which filter_scan turns into its prefix.
inline int filter_pix_blocks(int width, int height) { return (int)ceil_div((long long)width * height, vf::kPixBlock); }
struct FilterLayout {
    size_t off_table, off_flags, off_blk, bytes;
};
inline FilterLayout filter_layout(int max_ids, int width, int height) {
    FilterLayout l;
    l.off_table = 256;
    l.off_flags = l.off_table + ws_up((size_t)vf::kReplicas * max_ids * vf::kTableInts * sizeof(int));
    l.off_blk = l.off_flags + ws_up((size_t)width * height);
    l.bytes = l.off_blk + ws_up((size_t)filter_pix_blocks(width, height) * 2 * sizeof(int));
    return l;
}

// Instance tracker.  The workspace: the overflow word, the statistics of every detection row (int32 [vf::kReplicas][max_det]
// [vt::kStatInts]), the inside count of every pair (int32 [vf::kReplicas][max_pairs]; track_decide leaves the sum in copy 0), one byte
// of flags per pixel (valid, eroded) and the (emitted, out of grid) pair of every block of vf::kPixBlock pixels, as the filter's.
struct TrackLayout {
    size_t off_table, off_pairs, off_flags, off_blk, bytes;
};
inline TrackLayout track_layout(int max_det, int max_pairs, int width, int height) {
    TrackLayout l;
    l.off_table = 256;
    l.off_pairs = l.off_table + ws_up((size_t)vf::kReplicas * max_det * vt::kStatInts * sizeof(int));
    l.off_flags = l.off_pairs + ws_up((size_t)vf::kReplicas * max_pairs * sizeof(int));
    l.off_blk = l.off_flags + ws_up((size_t)width * height);
    l.bytes = l.off_blk + ws_up((size_t)filter_pix_blocks(width, height) * 2 * sizeof(int));
    return l;
}

// Depth tracker.  A maps buffer holds every level's map, level 0 first: level l is W_l x H_l entries of four floats (n0, n1, n2, d),
// width-major; W_l+1 = ceil(W_l / 2).  Offsets and the total are counted in entries of 16 bytes.
struct IcpLayout {
    int w[vi::kMaxLevels], h[vi::kMaxLevels];
    long long off[vi::kMaxLevels];
    long long entries;
};
inline IcpLayout icp_layout(int width, int height, int levels) {
    IcpLayout l;
    long long at = 0;
    for (int k = 0; k < vi::kMaxLevels; ++k) {
        l.w[k] = width; l.h[k] = height; l.off[k] = at;
        if (k < levels) at += (long long)width * height;
        width = (width + 1) / 2; height = (height + 1) / 2;
    }
    l.entries = at;
    return l;
}

// Visibility culling, the compaction of a mesh by a vertex mask.  The workspace: one byte per vertex (referenced by a kept face),
// the new index of every vertex (int32 [n_vertices], written by the emit call), and one int64 per block of vc::kCullWG faces and per
// block of vc::kCullWG vertices (the block's kept count, then - after cull_scan - its exclusive prefix).
struct CullLayout {
    int nfb, nvb; size_t off_newidx, off_fblk, off_vblk, bytes;
};
inline CullLayout cull_layout(long long n_vertices, long long n_faces) {
    CullLayout l;
    l.nfb = (int)ceil_div(n_faces, vc::kCullWG);
    l.nvb = (int)ceil_div(n_vertices, vc::kCullWG);
    l.off_newidx = ws_up((size_t)n_vertices);
    l.off_fblk = l.off_newidx + ws_up((size_t)n_vertices * sizeof(int));
    l.off_vblk = l.off_fblk + ws_up((size_t)l.nfb * sizeof(long long)) + 256;
    l.bytes = l.off_vblk + ws_up((size_t)l.nvb * sizeof(long long)) + 256;
    return l;
}

// Mesh components, the labelling.  The workspace: the union-find parents (int32 [n_vertices]), the dense number of every root
// (int32 [n_vertices], read only at roots) and one int64 per block of vcc::kCompWG vertices (the block's roots, then - after
// comp_scan - their exclusive prefix).  Faces need no workspace.
struct ComponentLayout {
    int nvb, nfb; size_t off_dense, off_vblk, bytes;
};
inline ComponentLayout component_layout(long long n_vertices, long long n_faces) {
    ComponentLayout l;
    l.nvb = (int)ceil_div(n_vertices, vcc::kCompWG);
    l.nfb = (int)ceil_div(n_faces, vcc::kCompWG);
    l.off_dense = ws_up((size_t)n_vertices * sizeof(int));
    l.off_vblk = l.off_dense + ws_up((size_t)n_vertices * sizeof(int));
    l.bytes = l.off_vblk + ws_up((size_t)l.nvb * sizeof(long long)) + 256;
    return l;
}

// The mesh rasteriser.  The workspace of the count call: per (view, block of vr::kRasterWG faces) an int64 pair - the block's large faces
// and their (view, face, tile) pairs, then (after raster_scan) their exclusive prefixes.  The large-face buffer the draw call fills:
// the first pair of every large face (int64 [large_cap]) and its record (vr::kLargeRecInts int32 each).
struct RasterLayout {
    int nfb; long long nblk; size_t bytes, off_rec, large_bytes;
};
inline RasterLayout raster_layout(long long n_faces, int n_views, long long large_cap) {
    RasterLayout l;
    l.nfb = (int)ceil_div(n_faces, vr::kRasterWG);
    l.nblk = (long long)l.nfb * n_views;
    l.bytes = ws_up((size_t)l.nblk * 2 * sizeof(long long)) + 256;
    l.off_rec = ws_up((size_t)large_cap * sizeof(long long)) + 256;
    l.large_bytes = l.off_rec + ws_up((size_t)large_cap * vr::kLargeRecInts * sizeof(int)) + 256;
    return l;
}

}  // namespace vl
