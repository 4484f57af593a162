"""ctypes binding of libvmapstep.so (C ABI in include/vmapstep.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is NO fallback: if the
shared object is missing or a call fails, the product path raises.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VMAPSTEP_LIBRARY", os.path.join(_HERE, "libvmapstep.so"))   # override: measurement builds only

NUM_FC = 14
ABI_VERSION = 7
WEIGHTS_F32, WEIGHTS_BF16 = 0, 1


KERNEL_AUTO, KERNEL_GEN, KERNEL_WIDE4, KERNEL_H32_F32, KERNEL_WS1, KERNEL_WP, KERNEL_S32_BWD6 = 0, 1, 2, 4, 5, 6, 8


class Tuning(ctypes.Structure):
    """vmapstep_tuning: measurement / test overrides of the automatic launch plan, passed per call through Shape.tuning."""
    _fields_ = [("workgroups_per_object", ctypes.c_int32), ("kernel", ctypes.c_int32), ("generic_finalize", ctypes.c_int32),
                ("ws_flags", ctypes.c_int32)]


class Shape(ctypes.Structure):
    _fields_ = [("n_obj", ctypes.c_int32), ("rays", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("hidden", ctypes.c_int32), ("weight_dtype", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("tuning", ctypes.POINTER(Tuning))]


class PlanInfo(ctypes.Structure):
    """vmapstep_plan_info (ABI v6): the launch plan the library derives from a shape."""
    _fields_ = [("kernel", ctypes.c_char * 48), ("rays_per_round", ctypes.c_int32), ("rounds_per_object", ctypes.c_int32),
                ("workgroups_per_object", ctypes.c_int32), ("tiles_per_round", ctypes.c_int32), ("waves_per_workgroup", ctypes.c_int32),
                ("single_round", ctypes.c_int32)]


class Tensor(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("obj_stride", ctypes.c_int64)]


class Params(ctypes.Structure):
    _fields_ = [("fc", Tensor * NUM_FC), ("pe_B", Tensor)]


class Batch(ctypes.Structure):
    _fields_ = [
        ("pcs", ctypes.c_void_p), ("pcs_stride", ctypes.c_int64 * 4),
        ("z", ctypes.c_void_p), ("z_stride", ctypes.c_int64 * 3),
        ("gt_depth", ctypes.c_void_p), ("gt_depth_stride", ctypes.c_int64 * 2),
        ("gt_rgb", ctypes.c_void_p), ("gt_rgb_stride", ctypes.c_int64 * 3),
        ("sem", ctypes.c_void_p), ("sem_stride", ctypes.c_int64 * 2),
        ("depth_mask", ctypes.c_void_p), ("depth_mask_stride", ctypes.c_int64 * 2),
        # ABI v7: the hand-off as rays (pcs == NULL): point = (ray_o + ray_d * z) - center
        ("ray_o", ctypes.c_void_p), ("ray_o_stride", ctypes.c_int64 * 3),
        ("ray_d", ctypes.c_void_p), ("ray_d_stride", ctypes.c_int64 * 3),
        ("center", ctypes.c_void_p), ("center_stride", ctypes.c_int64),
    ]


class Outputs(ctypes.Structure):
    _fields_ = [("loss", ctypes.c_void_p), ("flags", ctypes.c_void_p), ("render_depth", ctypes.c_void_p),
                ("render_color", ctypes.c_void_p), ("opacity", ctypes.c_void_p), ("var", ctypes.c_void_p),
                ("loss_terms", ctypes.c_void_p)]


class AdamW(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float), ("step", ctypes.c_int32),
                ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("bias_table", ctypes.c_void_p), ("table_len", ctypes.c_int32), ("step_counter", ctypes.c_void_p)]


class SampleObject(ctypes.Structure):
    _fields_ = [("rgbs", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("t_wc", ctypes.c_void_p), ("bbox", ctypes.c_void_p),
                ("n_keyframes", ctypes.c_int32), ("last2", ctypes.c_int32 * 2), ("center", ctypes.c_float * 3),
                ("obj_id", ctypes.c_int32), ("slots", ctypes.c_void_p), ("inst", ctypes.c_void_p)]


class SampleCfg(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("frames", ctypes.c_int32),
                ("samples_per_frame", ctypes.c_int32), ("n_bins_cam2surface", ctypes.c_int32), ("n_bins", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_depth", ctypes.c_float), ("surface_eps", ctypes.c_float), ("stop_eps", ctypes.c_float)]


class SampleRandoms(ctypes.Structure):
    _fields_ = [("kf_ids", ctypes.c_void_p), ("u_w", ctypes.c_void_p), ("u_h", ctypes.c_void_p), ("u_z", ctypes.c_void_p),
                ("g_z", ctypes.c_void_p)]


class SurfaceRandoms(ctypes.Structure):
    _fields_ = [("u0", ctypes.c_void_p), ("r", ctypes.c_void_p)]


class ViewCfg(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("samples", ctypes.c_int32), ("n_obj", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("t_wc", ctypes.c_float * 16), ("min_depth", ctypes.c_float), ("pix_begin", ctypes.c_int64), ("pix_end", ctypes.c_int64)]


VIEW_MAX_HITS = 16
VIEW_MAX_GROUPS = 4


class ViewGroup(ctypes.Structure):
    """vmapstep_view_group: one field group of a scene view (its hidden width, object count, samples per hit and stacked fields)."""
    _fields_ = [("hidden", ctypes.c_int32), ("n_obj", ctypes.c_int32), ("samples", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("params", ctypes.POINTER(Params)), ("pe_scale", ctypes.POINTER(Tensor))]


class IngestCfg(ctypes.Structure):
    """vmapstep_ingest_cfg: the frame shape, the input types and the labelling rules of one vmapstep_ingest_frame call."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("depth_f32", ctypes.c_int32), ("label_i32", ctypes.c_int32),
                ("depth_scale", ctypes.c_float), ("max_depth", ctypes.c_float), ("bbox_scale", ctypes.c_float),
                ("min_box", ctypes.c_int32), ("max_ids", ctypes.c_int32), ("n_background", ctypes.c_int32),
                ("background_classes", ctypes.c_int32 * 64)]


INGEST_MAX_CLASSES = 64
INGEST_ROW_INTS = 8                        # id, status, count, box[4], class
INGEST_ABSENT, INGEST_KEPT, INGEST_BACKGROUND, INGEST_SMALL, INGEST_ZERO_MARGIN, INGEST_MIXED = range(6)

class FilterCfg(ctypes.Structure):
    """vmapstep_filter_cfg: the frame shape, the input types, the camera and the rules of the vmapstep_filter_* calls of one frame."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("depth_f32", ctypes.c_int32), ("label_i32", ctypes.c_int32),
                ("depth_scale", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("t_wc", ctypes.c_float * 16), ("voxel_size", ctypes.c_float),
                ("id_shift", ctypes.c_int32), ("min_pixels", ctypes.c_int32), ("min_points", ctypes.c_int32),
                ("erode_radius", ctypes.c_int32), ("max_ids", ctypes.c_int32), ("n_background", ctypes.c_int32),
                ("background_classes", ctypes.c_int32 * 64)]


FILTER_MAX_CLASSES = 64
FILTER_ROW_INTS = 8                        # id, status, class, pixels, valid, inside, eroded, eroded_valid
FILTER_HEAD_INTS = 4                       # n_rows, overflow, n_keys, out_of_grid
FILTER_BOX_FLOATS = 16                     # centre, three axes, three half extents, known flag
FILTER_MAX_IDS = 32767
FILTER_MAX_RADIUS = 8


class TrackCfg(ctypes.Structure):
    """vmapstep_track_cfg: the frame shape, the input types, the camera, the rules and the frame's counts of the vmapstep_track_* calls."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("depth_f32", ctypes.c_int32), ("label_i32", ctypes.c_int32),
                ("depth_scale", ctypes.c_float), ("max_depth", ctypes.c_float),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("t_wc", ctypes.c_float * 16), ("voxel_size", ctypes.c_float),
                ("det_shift", ctypes.c_int32), ("min_pixels", ctypes.c_int32), ("min_points", ctypes.c_int32), ("erode_radius", ctypes.c_int32),
                ("max_det", ctypes.c_int32), ("max_pairs", ctypes.c_int32), ("max_ids", ctypes.c_int32),
                ("n_det", ctypes.c_int32), ("n_pairs", ctypes.c_int32), ("next_id", ctypes.c_int32), ("ratio_q", ctypes.c_int32),
                ("n_background", ctypes.c_int32), ("background_classes", ctypes.c_int32 * 64)]


TRACK_ROW_INTS = 9                         # d, status, class, persistent id, pixels, valid, inside, eroded, eroded_valid
TRACK_HEAD_INTS = 4                        # n_rows, overflow, n_keys, out_of_grid
TRACK_MAX_DET = 4096
TRACK_MAX_PAIRS = 65536
TRACK_PAIR_SLOTS = 64                      # pairs one track_stats workgroup holds in LDS; more go to global memory directly


class CullCfg(ctypes.Structure):
    """vmapstep_cull_cfg: the camera, the image size and the mode of one vmapstep_cull_mark call."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_depth", ctypes.c_float), ("occlusion_eps", ctypes.c_float),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("margin", ctypes.c_int32), ("use_depth", ctypes.c_int32)]


class RasterCfg(ctypes.Structure):
    """vmapstep_raster_cfg: the camera, the depth bounds and the image size of the vmapstep_raster_* calls."""
    _fields_ = [("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float), ("width", ctypes.c_int32), ("height", ctypes.c_int32)]


class IcpCfg(ctypes.Structure):
    """vmapstep_icp_cfg: the image size, the levels and their iteration counts, the camera and the thresholds of the vmapstep_icp_* calls."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("levels", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 4), ("grid_cap", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float), ("band", ctypes.c_float), ("dist_thresh", ctypes.c_float),
                ("cos_thresh", ctypes.c_float), ("reserved_f", ctypes.c_float),
                ("damping", ctypes.c_double), ("pivot_rel", ctypes.c_double), ("eps", ctypes.c_double)]


class TsdfCfg(ctypes.Structure):
    """vmapstep_tsdf_cfg: the volume's shape and affine, the object id, the camera, the image size and the rules of vmapstep_tsdf_integrate."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("obj_id", ctypes.c_int32),
                ("affine", ctypes.c_float * 12),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("margin", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float), ("trunc", ctypes.c_float), ("max_weight", ctypes.c_float)]


class RaycastCfg(ctypes.Structure):
    """vmapstep_raycast_cfg: the volume's shape, the image size, the camera, the depth range and the rules of vmapstep_tsdf_raycast."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("max_steps", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_depth", ctypes.c_float), ("max_depth", ctypes.c_float), ("step", ctypes.c_float), ("min_weight", ctypes.c_float),
                ("normal_map", ctypes.c_float * 9), ("reserved_f", ctypes.c_float)]


RAYCAST_IGNORE_BRICKS = 1
RAYCAST_MISS, RAYCAST_HIT, RAYCAST_LEFT, RAYCAST_BEHIND, RAYCAST_STEPS = 0, 1, 2, 3, 4
RAYCAST_MAX_STEPS = (1 << 24) - 1

ICP_MAX_LEVELS = 4
ICP_MAX_ITERATIONS = 64
ICP_MAX_PIXELS = 1 << 20                   # the bound under which the int64 sums cannot overflow (csrc/icp_rules.h)
ICP_SUMS = 29                              # inliers, 21 of J J^T, 6 of J r, r^2
ICP_LOG_COLS = 4                           # inlier count, sum of r^2, status, |x|^2
ICP_STATE_BYTES = 512
ICP_OK, ICP_DEGENERATE, ICP_SKIPPED = 0, 1, 2


EXPORTS = (
    "vmapstep_last_error", "vmapstep_abi_version", "vmapstep_param_layout", "vmapstep_workspace_bytes",
    "vmapstep_fwd_bwd", "vmapstep_render", "vmapstep_train_steps",
    "vmapstep_profile_main_kernel", "vmapstep_profile_phases", "vmapstep_prepare", "vmapstep_train_steps_prepared",
    "vmapstep_workspace_counts_offset", "vmapstep_fwd_bwd_prepared", "vmapstep_sample_frame",
    "vmapstep_query_workspace_bytes", "vmapstep_query_points", "vmapstep_profile_train_steps", "vmapstep_adamw_apply",
    "vmapstep_sample_workspace_bytes", "vmapstep_describe_plan", "vmapstep_sample_frame_rays",
    "vmapstep_mesh_workspace_bytes", "vmapstep_mesh_grid_points", "vmapstep_mesh_count", "vmapstep_mesh_emit",
    "vmapstep_nn_workspace_bytes", "vmapstep_nn_distance", "vmapstep_surface_sample_workspace_bytes", "vmapstep_surface_sample",
    "vmapstep_clip_box_workspace_bytes", "vmapstep_clip_box_count", "vmapstep_clip_box_emit",
    "vmapstep_unproject_workspace_bytes", "vmapstep_unproject_count", "vmapstep_unproject_emit", "vmapstep_obb_extents",
    "vmapstep_cloud_moments", "vmapstep_view_workspace_bytes", "vmapstep_view_count", "vmapstep_view_render",
    "vmapstep_scene_view_workspace_bytes", "vmapstep_scene_view_count", "vmapstep_scene_view_render",
    "vmapstep_ingest_workspace_bytes", "vmapstep_ingest_frame",
    "vmapstep_filter_workspace_bytes", "vmapstep_filter_stats", "vmapstep_filter_emit", "vmapstep_filter_write", "vmapstep_voxel_points",
    "vmapstep_track_workspace_bytes", "vmapstep_track_stats", "vmapstep_track_emit", "vmapstep_track_write",
    "vmapstep_cull_mark", "vmapstep_cull_workspace_bytes", "vmapstep_cull_faces_count", "vmapstep_cull_faces_emit",
    "vmapstep_components_workspace_bytes", "vmapstep_components_label", "vmapstep_components_stats",
    "vmapstep_raster_workspace_bytes", "vmapstep_raster_count", "vmapstep_raster_draw", "vmapstep_raster_resolve", "vmapstep_depth_compare",
    "vmapstep_icp_maps_bytes", "vmapstep_icp_pyramid", "vmapstep_icp_sums", "vmapstep_icp_track",
    "vmapstep_mesh_count_valid", "vmapstep_mesh_emit_valid", "vmapstep_tsdf_integrate",
    "vmapstep_tsdf_bricks_bytes", "vmapstep_tsdf_bricks", "vmapstep_tsdf_raycast",
)

_libs = {}


class VmapStepError(RuntimeError):
    pass


def load(path=None):
    """Load the HIP library (``path``: another build of it - the measurement build of tests/tools - next to the product's; each is
    loaded once). Import torch first so that its libamdhip64 is the one both sides share."""
    path = os.path.abspath(path or LIB_PATH)
    if path in _libs:
        return _libs[path]
    import torch  # noqa: F401  (maps torch/lib/libamdhip64.so before our NEEDED entry is resolved)
    if not os.path.exists(path):
        raise VmapStepError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU/PyTorch fallback for the training step.")
    lib = ctypes.CDLL(path)
    lib.vmapstep_last_error.restype = ctypes.c_char_p
    lib.vmapstep_abi_version.restype = ctypes.c_int
    lib.vmapstep_param_layout.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.vmapstep_workspace_bytes.argtypes = [ctypes.POINTER(Shape), ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_fwd_bwd.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                     ctypes.POINTER(Batch), ctypes.c_float, ctypes.c_float, ctypes.POINTER(Params),
                                     ctypes.POINTER(Outputs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_render.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                    ctypes.POINTER(Batch), ctypes.c_float, ctypes.c_float,
                                    ctypes.POINTER(Outputs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_train_steps.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                         ctypes.POINTER(Batch), ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                                         ctypes.c_float, ctypes.POINTER(AdamW), ctypes.POINTER(Params),
                                         ctypes.POINTER(Outputs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_prepare.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Batch), ctypes.c_int64,
                                     ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    lib.vmapstep_train_steps_prepared.argtypes = lib.vmapstep_train_steps.argtypes
    lib.vmapstep_fwd_bwd_prepared.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                              ctypes.POINTER(Batch), ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.POINTER(Params),
                                              ctypes.POINTER(Outputs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_adamw_apply.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.POINTER(AdamW), ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_float,
                                         ctypes.POINTER(Outputs), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_workspace_counts_offset.argtypes = [ctypes.POINTER(Shape), ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_sample_frame.argtypes = [ctypes.POINTER(SampleCfg), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(SampleRandoms), ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p]
    lib.vmapstep_sample_frame_rays.argtypes = [ctypes.POINTER(SampleCfg), ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(SampleRandoms), ctypes.c_void_p, ctypes.c_size_t,
                                               ctypes.c_void_p]
    lib.vmapstep_sample_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_query_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_query_points.argtypes = [ctypes.c_int32, ctypes.POINTER(Params), ctypes.POINTER(Tensor), ctypes.c_int32,
                                          ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_profile_train_steps.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                                 ctypes.POINTER(Batch), ctypes.c_int64, ctypes.c_int32, ctypes.c_float,
                                                 ctypes.c_float, ctypes.POINTER(AdamW), ctypes.POINTER(Outputs),
                                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    lib.vmapstep_profile_main_kernel.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                                 ctypes.POINTER(Batch), ctypes.c_int32, ctypes.c_void_p,
                                                 ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_profile_phases.argtypes = [ctypes.POINTER(Shape), ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                            ctypes.POINTER(Batch), ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]
    lib.vmapstep_describe_plan.argtypes = [ctypes.POINTER(Shape), ctypes.c_int32, ctypes.POINTER(PlanInfo)]
    lib.vmapstep_mesh_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_mesh_grid_points.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float),
                                              ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_mesh_count.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_mesh_emit.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                       ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_nn_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_nn_distance.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_surface_sample_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_surface_sample.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                            ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.POINTER(SurfaceRandoms),
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_clip_box_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_clip_box_count.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_float),
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_clip_box_emit.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_float),
                                           ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _unproject = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float),
                  ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32]
    lib.vmapstep_unproject_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_unproject_count.argtypes = _unproject + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_unproject_emit.argtypes = _unproject + [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_obb_extents.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_cloud_moments.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_view_workspace_bytes.argtypes = [ctypes.POINTER(ViewCfg), ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_view_count.argtypes = [ctypes.POINTER(ViewCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_view_render.argtypes = [ctypes.POINTER(ViewCfg), ctypes.c_int32, ctypes.POINTER(Params), ctypes.POINTER(Tensor),
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _scene = [ctypes.POINTER(ViewCfg), ctypes.POINTER(ViewGroup), ctypes.c_int32]
    lib.vmapstep_scene_view_workspace_bytes.argtypes = _scene + [ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_scene_view_count.argtypes = _scene + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_scene_view_render.argtypes = _scene + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64),
                                                        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_ingest_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_ingest_frame.argtypes = [ctypes.POINTER(IngestCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_filter_workspace_bytes.argtypes = [ctypes.POINTER(FilterCfg), ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_filter_stats.argtypes = [ctypes.POINTER(FilterCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_filter_emit.argtypes = [ctypes.POINTER(FilterCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_filter_write.argtypes = [ctypes.POINTER(FilterCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_voxel_points.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_float,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_track_workspace_bytes.argtypes = [ctypes.POINTER(TrackCfg), ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_track_stats.argtypes = [ctypes.POINTER(TrackCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_track_emit.argtypes = [ctypes.POINTER(TrackCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_track_write.argtypes = [ctypes.POINTER(TrackCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for fn in ("vmapstep_track_workspace_bytes", "vmapstep_track_stats", "vmapstep_track_emit", "vmapstep_track_write"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.vmapstep_cull_mark.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                       ctypes.POINTER(CullCfg), ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_cull_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_cull_faces_count.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_cull_faces_emit.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                             ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                             ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_components_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_components_label.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_components_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    _mesh_views = [ctypes.POINTER(RasterCfg), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_int32, ctypes.c_void_p]
    lib.vmapstep_raster_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int64, ctypes.POINTER(ctypes.c_size_t),
                                                    ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_raster_count.argtypes = _mesh_views + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_raster_draw.argtypes = _mesh_views + [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t,
                                                       ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_raster_resolve.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_depth_compare.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    for fn in ("vmapstep_raster_workspace_bytes", "vmapstep_raster_count", "vmapstep_raster_draw", "vmapstep_raster_resolve",
               "vmapstep_depth_compare"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.vmapstep_icp_maps_bytes.argtypes = [ctypes.POINTER(IcpCfg), ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_icp_pyramid.argtypes = [ctypes.POINTER(IcpCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.vmapstep_icp_sums.argtypes = [ctypes.POINTER(IcpCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]
    lib.vmapstep_icp_track.argtypes = [ctypes.POINTER(IcpCfg), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for fn in ("vmapstep_icp_maps_bytes", "vmapstep_icp_pyramid", "vmapstep_icp_sums", "vmapstep_icp_track"):
        getattr(lib, fn).restype = ctypes.c_int
    lib.vmapstep_mesh_count_valid.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_mesh_emit_valid.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float,
                                             ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.vmapstep_tsdf_integrate.argtypes = [ctypes.POINTER(TsdfCfg)] + [ctypes.c_void_p] * 8 + [ctypes.c_int32, ctypes.c_void_p]
    lib.vmapstep_tsdf_bricks_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    lib.vmapstep_tsdf_bricks.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float] + [ctypes.c_void_p] * 4
    lib.vmapstep_tsdf_raycast.argtypes = [ctypes.POINTER(RaycastCfg)] + [ctypes.c_void_p] * 5 + [ctypes.c_int32] + [ctypes.c_void_p] * 5
    for fn in ("vmapstep_mesh_count_valid", "vmapstep_mesh_emit_valid", "vmapstep_tsdf_integrate", "vmapstep_tsdf_bricks_bytes",
               "vmapstep_tsdf_bricks", "vmapstep_tsdf_raycast"):
        getattr(lib, fn).restype = ctypes.c_int
    for fn in ("vmapstep_filter_workspace_bytes", "vmapstep_filter_stats", "vmapstep_filter_emit", "vmapstep_filter_write",
               "vmapstep_voxel_points", "vmapstep_cull_mark", "vmapstep_cull_workspace_bytes", "vmapstep_cull_faces_count",
               "vmapstep_cull_faces_emit", "vmapstep_components_workspace_bytes", "vmapstep_components_label", "vmapstep_components_stats"):
        getattr(lib, fn).restype = ctypes.c_int
    for fn in ("vmapstep_unproject_workspace_bytes", "vmapstep_unproject_count", "vmapstep_unproject_emit", "vmapstep_obb_extents",
               "vmapstep_cloud_moments", "vmapstep_view_workspace_bytes", "vmapstep_view_count", "vmapstep_view_render",
               "vmapstep_scene_view_workspace_bytes", "vmapstep_scene_view_count", "vmapstep_scene_view_render",
               "vmapstep_ingest_workspace_bytes", "vmapstep_ingest_frame"):
        getattr(lib, fn).restype = ctypes.c_int
    for fn in ("vmapstep_describe_plan", "vmapstep_param_layout", "vmapstep_workspace_bytes", "vmapstep_fwd_bwd", "vmapstep_render",
               "vmapstep_train_steps", "vmapstep_profile_main_kernel",
               "vmapstep_profile_phases", "vmapstep_prepare", "vmapstep_train_steps_prepared",
               "vmapstep_workspace_counts_offset", "vmapstep_fwd_bwd_prepared", "vmapstep_sample_frame",
               "vmapstep_query_workspace_bytes", "vmapstep_query_points", "vmapstep_profile_train_steps", "vmapstep_adamw_apply",
               "vmapstep_sample_workspace_bytes", "vmapstep_sample_frame_rays", "vmapstep_mesh_workspace_bytes", "vmapstep_mesh_grid_points",
               "vmapstep_mesh_count", "vmapstep_mesh_emit", "vmapstep_nn_workspace_bytes", "vmapstep_nn_distance",
               "vmapstep_surface_sample_workspace_bytes", "vmapstep_surface_sample", "vmapstep_clip_box_workspace_bytes",
               "vmapstep_clip_box_count", "vmapstep_clip_box_emit"):
        getattr(lib, fn).restype = ctypes.c_int
    if lib.vmapstep_abi_version() != ABI_VERSION:
        raise VmapStepError(f"ABI mismatch: library {lib.vmapstep_abi_version()} != binding {ABI_VERSION}")
    _libs[path] = lib
    return lib


def describe_plan(n_obj: int, rays: int, samples: int, hidden: int, weights_bf16: bool = False, max_steps: int = 20, tuning: dict = None,
                  library: str = None) -> dict:
    """The launch plan for a shape as a dict (kernel name, rays per round, rounds / workgroups per object, tiles per round, waves per
    workgroup, single_round) - no device needed.  ``library``: the build to ask (default: the product library)."""
    lib = load(library)
    sh = Shape(n_obj, rays, samples, hidden, WEIGHTS_BF16 if weights_bf16 else WEIGHTS_F32)
    t = Tuning(**tuning) if tuning else None
    if t is not None:
        sh.tuning = ctypes.pointer(t)
    info = PlanInfo()
    check(lib.vmapstep_describe_plan(ctypes.byref(sh), max_steps, ctypes.byref(info)), lib)
    return {"kernel": info.kernel.decode(), **{k: int(getattr(info, k)) for k, _ in PlanInfo._fields_[1:]}}


def check(rc: int, lib):
    """Raise on a non-zero status; the message comes from the library that made the call (each build has its own thread-local
    last-error string)."""
    if rc != 0:
        msg = lib.vmapstep_last_error().decode("utf-8", "replace")
        raise VmapStepError(f"vmapstep error {rc}: {msg}")
