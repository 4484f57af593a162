"""Per-object model holder with the reference's attribute surface (trainer.py:9-33).

``Trainer(cfg)`` exposes ``fc_occ_map``, ``pe``, ``obj_scale``, ``device``, ``hidden_feature_size``, ``obj_id``
and ``bound_extent`` so that code written against the reference's ``sceneObject.trainer`` keeps working.
``cfg`` is any object with the attributes the reference's ``cfg.Config`` provides (cfg.py:6-91).
``meshing`` (trainer.py:35-75) and ``eval_points`` run on the device: the dense grid, the occupancy query, marching cubes
(vmap_amd/meshing.py; its docstring lists the deviations from the reference's skimage / trimesh path) and the colour query.
"""
from __future__ import annotations

import torch

from . import fields, layout


class Trainer:
    def __init__(self, cfg):
        self.obj_id = cfg.obj_id
        self.device = cfg.training_device
        self.hidden_feature_size = cfg.hidden_feature_size
        self.obj_scale = cfg.obj_scale
        self.n_unidir_funcs = cfg.n_unidir_funcs
        self.emb_size1 = layout.EMB1
        self.emb_size2 = layout.EMB2
        self.load_network()
        self.bound_extent = 0.995 if self.obj_id == 0 else 0.9      # trainer.py:21-24

    def load_network(self):
        self.fc_occ_map = fields.OccupancyMap(self.emb_size1, self.emb_size2, hidden_size=self.hidden_feature_size)
        self.fc_occ_map.apply(fields.init_weights).to(self.device)
        self.pe = fields.UniDirsEmbed(max_deg=self.n_unidir_funcs, scale=self.obj_scale).to(self.device)

    @torch.no_grad()
    def meshing(self, bound, obj_center, grid_dim=256, min_component_area=None, largest_components=None):
        """The reference's Trainer.meshing (trainer.py:35-75) on the device: grid_dim^3 grid points of the object box (scale
        bound.extent / (2 bound_extent), rotation bound.R, centre bound.center, minus obj_center) -> eval_points -> marching cubes at
        0.5 with the vertices mapped to scene coordinates (obj_center NOT subtracted, as in the reference) -> eval_points at the
        vertices -> colours (color * 255) truncated to uint8.  ``bound``: anything with .extent, .center, .R (meshing.BoundingBox,
        an open3d OrientedBoundingBox).  Returns a meshing.Mesh, or None where the reference returns None.

        ``min_component_area`` (m^2) and / or ``largest_components`` (k) drop floaters (``components.keep_components``) after
        marching cubes and BEFORE the colour query, so a dropped vertex is never queried; ``None`` when nothing is left.  Both
        off (the default): the reference's behaviour."""
        from . import meshing
        D = int(grid_dim)
        dev = torch.device(self.device)
        pts = meshing.grid_points((D, D, D), meshing.bound_affine(bound, self.bound_extent, D, obj_center), dev)
        ret = self.eval_points(pts)
        if ret is None:
            return None
        occ, _ = ret
        del pts
        mesh = meshing.extract_mesh(occ.view(D, D, D), 0.5, meshing.bound_affine(bound, self.bound_extent, D))
        if mesh is None:
            return None
        if min_component_area is not None or largest_components is not None:
            from . import components
            with torch.cuda.device(dev):
                mesh = components.keep_components(mesh, min_area=0.0 if min_component_area is None else min_component_area,
                                                  largest=largest_components)
            if mesh is None:
                return None
        ret = self.eval_points(mesh.vertices)
        if ret is None:
            return None
        _, color = ret
        mesh.vertex_colors = (color * 255).to(torch.uint8)
        return mesh

    @torch.no_grad()
    def eval_points(self, points: torch.Tensor, chunk_size: int = 100000):
        """Occupancy and colour at arbitrary points of this object's frame (trainer.py:77-95): ONE launch of the HIP query
        kernel (vmapstep_query_points).  There is no CPU / PyTorch-ops path: points on another device, or a hidden width
        the kernels do not implement, raise (``chunk_size`` is accepted for signature compatibility and unused)."""
        from . import _lib
        if not points.is_cuda:
            raise _lib.VmapStepError("Trainer.eval_points runs on the GPU only (no CPU fallback): move the points to the training device")
        if self.hidden_feature_size % 32 != 0 or not 32 <= self.hidden_feature_size <= 256:
            raise _lib.VmapStepError(f"hidden width {self.hidden_feature_size}: supported widths are multiples of 32 up to 256")
        occ, color = self._eval_points_hip(points)
        if occ.max() == 0:
            return None
        return occ, color

    @torch.no_grad()
    def render_view(self, bound, obj_center, t_wc, intrinsics, width, height, **kw):
        """This object alone seen from the camera-to-world pose ``t_wc``: ``render.render_view`` with one field, its box ``bound``
        (anything with .center, .R, .extent) and its ``obj_center``.  Any hidden width 32, 64, ..., 256; GPU only."""
        from . import render
        return render.render_view([self], [bound], t_wc, intrinsics, width, height, centers=[obj_center], **kw)

    @torch.no_grad()
    def track_pose(self, depth, t_wc_init, bound, obj_center, intrinsics, *, min_opacity=0.5, samples=16, iterations=(10, 5, 4), **cfg):
        """The camera-to-world pose of the depth image ``depth`` ([W, H]) against this object's field: ``render_view`` from
        ``t_wc_init`` is the model (depth zeroed where the opacity is below ``min_opacity``), ``odometry.DepthTracker.track_to_view``
        aligns the frame to it.  -> ``odometry.TrackedPose``; ``cfg``: ``odometry.track_depth``'s keyword arguments.  GPU only."""
        from . import odometry
        width, height = (int(s) for s in depth.shape)
        view = self.render_view(bound, obj_center, t_wc_init, intrinsics, width, height, samples=samples)
        return odometry.DepthTracker(intrinsics, width, height, iterations, **cfg).track_to_view(view, depth, min_opacity, t_wc=t_wc_init)

    def _eval_points_hip(self, points: torch.Tensor):
        import ctypes
        from . import _lib
        lib = _lib.load()
        pts = points if points.dtype == torch.float32 else points.float()
        n = pts.shape[0]
        dev = pts.device
        nb = ctypes.c_size_t(0)
        _lib.check(lib.vmapstep_query_workspace_bytes(self.hidden_feature_size, ctypes.byref(nb)), lib)
        ws = torch.empty(nb.value + 256, dtype=torch.uint8, device=dev)
        ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
        pp = _lib.Params()
        for t, p in enumerate(self.fc_occ_map.parameters()):
            if not p.is_contiguous() or p.device != dev:
                raise ValueError("field parameters must be contiguous and on the points' device")
            pp.fc[t] = _lib.Tensor(p.data_ptr(), 0)
        pp.pe_B = _lib.Tensor(self.pe.B_layer.weight.data_ptr(), 0)
        scale = self.pe.scale.reshape(1).to(dev, torch.float32).contiguous()
        sc = _lib.Tensor(scale.data_ptr(), 0)
        occ = torch.empty(n, dtype=torch.float32, device=dev)
        col = torch.empty(n, 3, dtype=torch.float32, device=dev)
        strides = (ctypes.c_int64 * 2)(pts.stride(0), pts.stride(1))
        _lib.check(lib.vmapstep_query_points(self.hidden_feature_size, ctypes.byref(pp), ctypes.byref(sc), 0, pts.data_ptr(), n,
                                             strides, occ.data_ptr(), col.data_ptr(), ws_ptr, nb.value,
                                             torch.cuda.current_stream(dev).cuda_stream), lib)
        return occ, col


class SimpleConfig:
    """The subset of cfg.Config (cfg.py) the hot path reads, with the Replica room0 vMAP values as defaults."""

    def __init__(self, **kw):
        self.obj_id = -1
        self.training_device = "cuda:0"
        self.data_device = "cuda:0"
        self.training_strategy = "hip"        # third option next to the reference's "vmap" / "forloop" (cfg.py:20)
        self.hidden_feature_size = 32
        self.hidden_feature_size_bg = 128
        self.obj_scale = 2.0
        self.bg_scale = 5.0
        self.n_unidir_funcs = 5
        self.n_per_optim = 120
        self.n_per_optim_bg = 1200
        self.n_iter_per_frame = 20
        self.win_size = 5
        self.n_samples_per_frame = self.n_per_optim // self.win_size
        self.n_bins_cam2surface = 1
        self.n_bins_cam2surface_bg = 5
        self.n_bins = 9
        self.learning_rate = 1e-3
        self.weight_decay = 0.013
        self.do_bg = False
        for k, v in kw.items():
            setattr(self, k, v)
