// launch_geometry.h - the launch geometry of the mesh, evaluation and bounds families: the constants that both the kernels
// (mesh_kernels.h, eval_kernels.h, bounds_kernels.h) and the host-side workspace layouts and launch plans (launch.h) are built on.
// constexpr values only, no device code: the C ABI unit sizes workspaces from them without compiling anyone's kernels.
#pragma once

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
