"""TEST INFRASTRUCTURE: builds and loads the CPU SIMT executor build of the kernel headers (tests/sim)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = os.path.join(HERE, "sim")
OUT = os.path.join(SIM, "_build", "libvmsim.so")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


UNITS = ("sim_abi", "sim_runtime", "sim_k_f32", "sim_k_s32", "sim_k_ws", "sim_k_ws8", "sim_k_wp", "sim_k_misc", "sim_k_mesh", "sim_k_eval", "sim_k_bounds",
         "sim_hazard")


def _deps(src, pool):
    """The files of `pool` a source includes, transitively (by base name)."""
    import re
    by_name = {os.path.basename(h): h for h in pool}
    seen, todo = set(), [src]
    while todo:
        with open(todo.pop()) as fh:
            for inc in re.findall(r'#include\s+[<"]([^">]+)[">]', fh.read()):
                h = by_name.get(os.path.basename(inc))
                if h and h not in seen:
                    seen.add(h)
                    todo.append(h)
    return sorted(seen)


def build(force=False):
    """One object per kernel family (like the device build), compiled side by side by the host compiler, linked into
    tests/sim/_build/libvmsim.so; a unit is rebuilt only when one of the headers it includes changed."""
    csrc = os.path.join(ROOT, "vmap_amd", "csrc")
    pool = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + \
           [os.path.join(SIM, f) for f in os.listdir(SIM) if f.endswith(".h")] + [os.path.join(SIM, "include", "hip", "hip_runtime.h")]
    # the sim's wave_ops.h and fake <hip/hip_runtime.h> shadow the device ones (include order below)
    pool = [h for h in pool if h != os.path.join(csrc, "wave_ops.h")]
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    cxx = CLANG if os.path.exists(CLANG) else "clang++"
    flags = [cxx, "-std=c++17", "-O2", "-mfma", "-ffp-contract=fast-honor-pragmas", "-fPIC", "-pthread", "-I", SIM, "-I", os.path.join(SIM, "include"),
             "-I", csrc, "-Wno-unused-value", "-Wno-psabi", "-Wno-pass-failed"]
    # what the library is built from, by content: a library whose stamp matches is used as it is, whatever the files' times say
    # (a tree copied to another machine keeps its libraries but not its objects, and not necessarily its time stamps)
    import hashlib
    unit_deps = {u: [os.path.join(SIM, u + ".cpp"), os.path.abspath(__file__)] + _deps(os.path.join(SIM, u + ".cpp"), pool) for u in UNITS}
    # paths relative to the tree: the stamp holds wherever the tree lies
    h = hashlib.sha256(" ".join([os.path.relpath(f, ROOT) if os.path.isabs(f) else f for f in flags[1:]] + list(UNITS)).encode())
    for d in sorted({d for deps in unit_deps.values() for d in deps}):
        with open(d, "rb") as fh:
            h.update(os.path.relpath(d, ROOT).encode() + b"\0" + fh.read())
    stamp, digest = OUT + ".stamp", h.hexdigest()
    if not force and os.path.exists(OUT) and os.path.exists(stamp) and open(stamp).read() == digest:
        return OUT
    procs, objs = [], []
    for u in UNITS:
        src, obj = os.path.join(SIM, u + ".cpp"), os.path.join(os.path.dirname(OUT), u + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or any(os.path.getmtime(obj) < os.path.getmtime(d) for d in unit_deps[u]):
            procs.append((u, subprocess.Popen(flags + ["-c", src, "-o", obj])))
    failed = [u for u, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, f"simulator build: {failed}")
    subprocess.run([cxx, "-shared", "-fPIC", "-pthread", "-o", OUT + ".tmp"] + objs, check=True)
    os.replace(OUT + ".tmp", OUT)
    with open(stamp, "w") as fh:
        fh.write(digest)
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _p(a, ty=ctypes.c_float):
    return a.ctypes.data_as(ctypes.POINTER(ty)) if a is not None else None


FAMILIES = ("h32", "s32", "s32_bwd6", "gen", "wide", "ws", "wp")      # vl::Family, in its order


def step_plan(shape, max_steps, measurement_build):
    """The plan vl::make_plan (csrc/step_plan.h, as the executor library compiles it) makes for a vmap_amd._lib.Shape:
    -> (status, message, dict of family, G, tiles, NG, NW, PR, xcd_main, xcd_finalize, the section offsets and total - or None)"""
    out, msg = (ctypes.c_longlong * 18)(), ctypes.create_string_buffer(512)
    rc = lib().vmsim_step_plan(ctypes.byref(shape), int(max_steps), int(measurement_build), out, msg, len(msg))
    return rc, msg.value.decode(), None if rc else dict(zip(PLAN_FIELDS, out), family=FAMILIES[out[0]])


PLAN_FIELDS = ("family", "G", "tiles", "NG", "NW", "PR", "xcd_main", "xcd_finalize", "off_ploss", "off_imgtab", "off_tab_wt", "off_row_tab",
               "off_pgrad", "off_wimg", "off_scratch", "off_flags", "off_stats", "total")


def sim_step(case_or_fc, B=None, scale=None, batch=None, G=None, bwd=True, adam=None, NW=0, xcd_affine=1, weights_bf16=0, wide=False,
             split=False, rays=None, finalize_form=0):
    """Run prep + main + finalize on the simulator. Returns dict like oracle.training_step.
    split: hidden 32 on the split-bf16 kernels (step_prep_s32 / step_main_s32 / step_finalize_s32).
    rays: (origins [n,R,3], dirs [n,R,3], centres [n,3] or None) - the ABI v7 ray hand-off: the kernels get NO points tensor and rebuild
    the sample points themselves (load_point, csrc/step_kernels.h)."""
    if isinstance(case_or_fc, dict):
        c = case_or_fc
        fc, B, scale, batch = c["fc"], c["B"], c["scale"], c["batch"]
    else:
        fc = case_or_fc
    n, R, S = batch["z"].shape
    H = fc[2].shape[-1]
    if G is None:
        G = max(1, (32 if wide in (True, 1) else 64 if wide in (3, 4) else 128) // S)
    lib().vmsim_set_finalize_form(int(finalize_form))   # step_finalize_ws: 0 a thread per quad and row group, 1 one thread per quad (the library's choice for many blocks / few rows)
    # the kernel family (vl::Family, csrc/step_plan.h).  hidden 32 by split: 0 exact fp32 (step_main_h32), 1 step_main_s32, 2 step_main_s32
    # with the six-product backward; other widths by wide: 1 / True step_main_wide<4>, 3 step_main_ws (hidden 64 / 128 / 256), 4
    # step_main_wp (hidden 64 / 128), anything else - and a width the asked-for kernel does not have - the general kernel
    if H == 32:
        family = FAMILIES.index(("h32", "s32", "s32_bwd6")[int(split)])
    else:
        family = FAMILIES.index("wide" if int(wide) == 1 else "ws" if int(wide) == 3 and H in (64, 128, 256) else
                                "wp" if int(wide) == 4 and H in (64, 128) else "gen")
    fc_c = [np.ascontiguousarray(a, dtype=np.float32) for a in fc]
    sizes = [a[0].size for a in fc_c]
    P = sum(sizes) + 63
    PP = (P + 63) // 64 * 64
    arr = (ctypes.POINTER(ctypes.c_float) * 14)(*[_p(a) for a in fc_c])
    Bc = np.ascontiguousarray(B, dtype=np.float32)
    sc = np.ascontiguousarray(scale, dtype=np.float32)
    pcs = np.ascontiguousarray(batch["pcs"], dtype=np.float32)
    z = np.ascontiguousarray(batch["z"], dtype=np.float32)
    gd = np.ascontiguousarray(batch["gt_depth"], dtype=np.float32)
    rgb = np.ascontiguousarray(batch["gt_rgb"], dtype=np.float32)
    sem = np.ascontiguousarray(batch["sem"], dtype=np.uint8)
    dm = np.ascontiguousarray(batch["depth_mask"], dtype=np.uint8)
    grads = np.full((n, P), np.nan, dtype=np.float32)
    loss = np.full((1,), np.nan, dtype=np.float32)
    dD = np.full((n, R), np.nan, dtype=np.float32)
    dC = np.full((n, R, 3), np.nan, dtype=np.float32)
    dO = np.full((n, R), np.nan, dtype=np.float32)
    dV = np.full((n, R), np.nan, dtype=np.float32)
    flags = np.full((4,), -1, dtype=np.int32)
    do_adam, p_out, m, v, step, lr, wd = 0, None, None, None, 1, 1e-3, 0.013
    if adam is not None:
        do_adam = 1
        p_out, m, v, step = adam["p"], adam["m"], adam["v"], adam["step"]
    ray_keep = None
    if rays is not None:
        ray_keep = [np.ascontiguousarray(x, dtype=np.float32) if x is not None else None for x in rays]
        lib().vmsim_set_rays.argtypes = [ctypes.POINTER(ctypes.c_float)] * 3
        lib().vmsim_set_rays(_p(ray_keep[0]), _p(ray_keep[1]), _p(ray_keep[2]))
        pcs = np.full_like(pcs, np.nan)              # must not be read
    try:
        rc = lib().vmsim_step(
        n, R, S, H, family, G, int(NW), int(xcd_affine), int(weights_bf16), arr, _p(Bc), _p(sc), _p(pcs), _p(z), _p(gd), _p(rgb),
        _p(sem, ctypes.c_uint8), _p(dm, ctypes.c_uint8), ctypes.c_float(5.0), ctypes.c_float(10.0),
        _p(grads), _p(loss), _p(dD), _p(dC), _p(dO), _p(dV), _p(flags, ctypes.c_int), int(bool(bwd)),
        do_adam, _p(p_out), _p(m), _p(v), int(step), ctypes.c_float(lr), ctypes.c_float(wd))
    finally:
        if rays is not None:
            lib().vmsim_set_rays(None, None, None)
    if rc != 0:
        raise RuntimeError(f"vmsim_step failed: {rc}")
    out = dict(loss=float(loss[0]), render_depth=dD, render_color=dC, opacity=dO, var=dV, flags=flags, grads_flat=grads)
    o = 0
    for t, a in enumerate(fc_c):
        out[f"g_fc{t}"] = grads[:, o:o + sizes[t]].reshape(a.shape)
        o += sizes[t]
    out["g_B"] = grads[:, o:o + 63].reshape(n, 21, 3)
    return out


class _SimSampleObject(ctypes.Structure):
    _fields_ = [("rgbs", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("t_wc", ctypes.c_void_p), ("bbox", ctypes.c_void_p),
                ("n_keyframes", ctypes.c_int32), ("last2", ctypes.c_int32 * 2), ("center", ctypes.c_float * 3),
                ("obj_id", ctypes.c_int32), ("slots", ctypes.c_void_p), ("inst", ctypes.c_void_p)]


def sim_sample(scenes, rnds, seed=0, frame_counter=0, eps=0.1, stop_eps=0.05, nsplit=0):
    """Run frame_sample on the simulator for a list of scenes (same W,H,F,P,n1,n2); rnds = list of per-ray random dicts
    (test mode) or None (Philox mode).  nsplit > 1: the split form (frame_depth_max + frame_sample over ray slices).
    Returns dict of arrays with a leading object dimension."""
    L = lib()
    L.vmsim_set_sample_split(int(nsplit))
    assert L.vmsim_sample_object_size() == ctypes.sizeof(_SimSampleObject)
    n = len(scenes)
    s0 = scenes[0]
    W, H, F, P, n1, n2 = (s0[k] for k in ("W", "H", "F", "P", "n1", "n2"))
    S, FP = n1 + n2, F * P
    keep = []
    table = (_SimSampleObject * n)()
    for i, sc in enumerate(scenes):
        if "store" in sc:      # shared frame store: dict(rgbx u8 [C,W,H,4], depth, inst i32, t_wc) + slots i32 [K] + obj_id
            st = sc["store"]
            arrs = [np.ascontiguousarray(st["rgbx"], dtype=np.uint8), np.ascontiguousarray(st["depth"], dtype=np.float32),
                    np.ascontiguousarray(st["t_wc"], dtype=np.float32), np.ascontiguousarray(sc["bbox"], dtype=np.float32),
                    np.ascontiguousarray(sc["slots"], dtype=np.int32), np.ascontiguousarray(st["inst"], dtype=np.int32)]
            keep.append(arrs)
            table[i] = _SimSampleObject(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data,
                                        sc["K"], (ctypes.c_int32 * 2)(*sc["last2"]), (ctypes.c_float * 3)(*[float(v) for v in sc["center"]]),
                                        int(sc["obj_id"]), arrs[4].ctypes.data, arrs[5].ctypes.data)
            continue
        arrs = [np.ascontiguousarray(sc[k]) for k in ("rgbs", "depth", "t_wc", "bbox")]
        keep.append(arrs)
        table[i] = _SimSampleObject(arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data, arrs[3].ctypes.data,
                                    sc["K"], (ctypes.c_int32 * 2)(*sc["last2"]), (ctypes.c_float * 3)(*[float(v) for v in sc["center"]]),
                                    0, None, None)
    def cat(key, dt):
        if rnds is None:
            return None
        return np.ascontiguousarray(np.stack([r[key] for r in rnds]).astype(dt))
    kf, uw, uh, uz, gz = cat("kf_ids", np.int32), cat("u_w", np.float32), cat("u_h", np.float32), cat("u_z", np.float32), cat("g_z", np.float32)
    out = dict(pcs=np.full((n, FP, S, 3), np.nan, np.float32), z=np.full((n, FP, S), np.nan, np.float32),
               gt_depth=np.full((n, FP), np.nan, np.float32), gt_rgb=np.full((n, FP, 3), np.nan, np.float32),
               sem=np.full((n, FP), 255, np.uint8), depth_mask=np.full((n, FP), 255, np.uint8))
    fx, fy, cx, cy = s0["intr"]
    rc = L.vmsim_sample(table, n, W, H, F, P, n1, n2, ctypes.c_float(fx), ctypes.c_float(fy), ctypes.c_float(cx), ctypes.c_float(cy),
                        ctypes.c_float(s0["min_bound"]), ctypes.c_float(eps), ctypes.c_float(stop_eps),
                        ctypes.c_ulonglong(seed), ctypes.c_uint(frame_counter),
                        _p(kf, ctypes.c_int32), _p(uw), _p(uh), _p(uz), _p(gz),
                        _p(out["pcs"]), _p(out["z"]), _p(out["gt_depth"]), _p(out["gt_rgb"]),
                        _p(out["sem"], ctypes.c_uint8), _p(out["depth_mask"], ctypes.c_uint8))
    assert rc == 0
    return out


def sim_query(fc_k, B_k, scale_k, pts, grid=3, H=32):
    """field_query_h32 on the simulator for one object: fc_k = 14 arrays (no object dim), pts [N,3]."""
    fc_c = [np.ascontiguousarray(a, dtype=np.float32) for a in fc_k]
    arr = (ctypes.POINTER(ctypes.c_float) * 14)(*[_p(a) for a in fc_c])
    Bc = np.ascontiguousarray(B_k, dtype=np.float32)
    sc = np.ascontiguousarray([scale_k], dtype=np.float32)
    p = np.ascontiguousarray(pts, dtype=np.float32)
    n = p.shape[0]
    occ = np.full(n, np.nan, np.float32)
    rgb = np.full((n, 3), np.nan, np.float32)
    rc = lib().vmsim_query(arr, _p(Bc), _p(sc), _p(p), ctypes.c_longlong(n), _p(occ), _p(rgb), int(grid), int(H))
    assert rc == 0
    return occ, rgb


# ---- mesh extraction, mesh evaluation, object bounds (sim_k_mesh.cpp, sim_k_eval.cpp, sim_k_bounds.cpp) --------------------------------
# Every output and every workspace the kernels get is a _Buf: filled with POISON bytes and surrounded by guard regions of the same
# pattern, which check() requires to be untouched.  A kernel that writes past a capacity, or before a buffer, fails the wrapper.

POISON = 0xA5
GUARD = 4096
POISON_F32 = np.frombuffer(bytes([POISON] * 4), np.float32)[0]
POISON_I32 = np.frombuffer(bytes([POISON] * 4), np.int32)[0]
POISON_I64 = np.frombuffer(bytes([POISON] * 8), np.int64)[0]


class _Buf:
    def __init__(self, shape, dtype):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        self.raw = np.full(self.nbytes + 2 * GUARD + 256, POISON, np.uint8)
        self.off = GUARD + (-(self.raw.ctypes.data + GUARD)) % 256
        self.a = self.raw[self.off:self.off + self.nbytes].view(dtype).reshape(shape)
        self.ptr = ctypes.c_void_p(self.raw.ctypes.data + self.off)

    def check_sections(self, used, what=""):
        """used: (offset, bytes) of every section of a workspace; every byte outside them - the padding up to the next 256-byte
        boundary, the spare bytes a layout adds - must still be POISON: a section written past its end shows here."""
        free = np.ones(self.nbytes, bool)
        for off, n in used:
            free[int(off):int(off) + int(n)] = False
        bad = np.flatnonzero(free & (self.raw[self.off:self.off + self.nbytes] != POISON))
        assert bad.size == 0, f"{what}: workspace byte {int(bad[0])} between its sections was written"
        self.check(what)

    def check(self, what=""):
        before, after = self.raw[:self.off], self.raw[self.off + self.nbytes:]
        assert (before == POISON).all(), f"{what}: written before the buffer"
        assert (after == POISON).all(), f"{what}: written past the buffer ({int(np.flatnonzero(after != POISON)[0])} bytes past its end)"


def isolated(fn):
    """fn() in a forked child, its (picklable) result handed back: a kernel that dies on the host - SIGFPE, SIGSEGV - becomes an
    AssertionError of the calling test, not the end of the test run.  An exception in the child is raised again here."""
    import pickle
    import traceback
    rd, wr = os.pipe()
    pid = os.fork()
    if pid == 0:
        code = 0
        try:
            os.close(rd)
            try:
                payload = pickle.dumps((True, fn()), protocol=pickle.HIGHEST_PROTOCOL)
            except BaseException as e:      # noqa: BLE001 - reported in the parent
                payload = pickle.dumps((False, f"{type(e).__name__}: {e}\n{traceback.format_exc()}"))
            with os.fdopen(wr, "wb") as fh:
                fh.write(payload)
        except BaseException:               # noqa: BLE001
            code = 1
        finally:
            os._exit(code)
    os.close(wr)
    with os.fdopen(rd, "rb") as fh:
        data = fh.read()
    _, status = os.waitpid(pid, 0)
    if os.WIFSIGNALED(status):
        raise AssertionError(f"the kernel died on the executor with signal {os.WTERMSIG(status)}")
    if not data or os.WEXITSTATUS(status) != 0:
        raise AssertionError(f"the executor's child process ended with status {status} and no result")
    ok, value = pickle.loads(data)
    if not ok:
        raise AssertionError("in the executor's child process: " + value)
    return value


def set_schedule(s):
    """0: round-robin (the default); 1 / 2: wave-greedy, forward / reverse (tests/sim/sim_runtime.h)."""
    lib().vmsim_set_schedule(int(s))


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _ll(*v):
    return (ctypes.c_longlong * len(v))(*v)


def sim_scan_hazard(one_wsum, x, y):
    """The self-test kernels of sim_hazard.cpp: two workgroup scans in a row, through one wsum (wrong) or two. -> (ex, ey, totals)."""
    n = lib().vmsim_scan_hazard_lanes()
    x, y = _c(x, np.int32), _c(y, np.int32)
    assert len(x) == len(y) == n
    ex, ey, tot = _Buf(n, np.int32), _Buf(n, np.int32), _Buf((n, 2), np.int32)
    lib().vmsim_scan_hazard(int(one_wsum), _vp(x), _vp(y), ex.ptr, ey.ptr, tot.ptr)
    for b in (ex, ey, tot):
        b.check("scan_hazard")
    return ex.a, ey.a, tot.a


def mesh_layout(shape):
    out = _ll(0, 0, 0, 0, 0)
    lib().vmsim_mesh_layout(int(shape[0]), int(shape[1]), int(shape[2]), out)
    return dict(n=out[0], nblk=out[1], off_firstv=out[2], off_emask=out[3], bytes=out[4])


def ninv_of(affine):
    """The inverse transpose of the affine's linear part as the C ABI forms it: float64 adjugate / determinant of the float32 entries."""
    m = np.asarray(affine, np.float32).astype(np.float64)[:, :3]
    adj = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    det = m[0, 0] * adj[0, 0] + m[0, 1] * adj[1, 0] + m[0, 2] * adj[2, 0]
    return np.ascontiguousarray((adj / det).T, dtype=np.float32)


def sim_mesh(vol, level=0.5, affine=None, normals=True, n_vertices=None, n_faces=None):
    """mesh_count -> mesh_scan -> mesh_emit_vertices -> mesh_emit_faces.  n_vertices / n_faces: the capacities (default: the totals).
    -> dict(counts int64 [2], vertices [cap,3], normals [cap,3] or None, faces [capf,3], blk int64 [nblk,2], firstv, emask)"""
    L = lib()
    vol = _c(vol, np.float32)
    nx, ny, nz = vol.shape
    lay = mesh_layout(vol.shape)
    ws, counts = _Buf(lay["bytes"], np.uint8), _Buf(2, np.int64)
    L.vmsim_mesh_count(_vp(vol), nx, ny, nz, ctypes.c_float(level), counts.ptr, ws.ptr)
    sections = [(0, lay["nblk"] * 16), (lay["off_firstv"], 4 * lay["n"]), (lay["off_emask"], lay["n"])]
    ws.check_sections(sections, "mesh workspace after count"), counts.check("mesh counts")
    nv, nf = (int(c) for c in counts.a)
    cv, cf = nv if n_vertices is None else int(n_vertices), nf if n_faces is None else int(n_faces)
    verts, faces = _Buf((cv, 3), np.float32), _Buf((cf, 3), np.int32)
    norm = _Buf((cv, 3), np.float32) if normals else None
    A = _c(affine, np.float32) if affine is not None else None
    Ni = ninv_of(affine) if affine is not None else None
    L.vmsim_mesh_emit(_vp(vol), nx, ny, nz, ctypes.c_float(level), _vp(A), _vp(Ni), verts.ptr, norm.ptr if norm else None, faces.ptr,
                      ctypes.c_longlong(cv), ctypes.c_longlong(cf), ws.ptr)
    ws.check_sections(sections, "mesh workspace")
    for b, w in ((verts, "vertices"), (faces, "faces")) + (((norm, "normals"),) if norm else ()):
        b.check(w)
    nblk, n = lay["nblk"], lay["n"]
    return dict(counts=counts.a.copy(), vertices=verts.a, normals=norm.a if norm else None, faces=faces.a,
                blk=ws.a[:nblk * 16].view(np.int64).reshape(nblk, 2),
                firstv=ws.a[lay["off_firstv"]:lay["off_firstv"] + 4 * n].view(np.int32),
                emask=ws.a[lay["off_emask"]:lay["off_emask"] + n])


def sim_mesh_grid_points(shape, affine):
    n = int(np.prod(shape))
    out = _Buf((n, 3), np.float32)
    A = _c(affine, np.float32)
    lib().vmsim_mesh_grid_points(int(shape[0]), int(shape[1]), int(shape[2]), _vp(A), out.ptr)
    out.check("grid points")
    return out.a


def _offsets(counts, n):
    if counts is None:
        return np.array([0, n], np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def sim_nn(q, r, qo=None, ro=None, rchunk=0, q_begin=None, q_end=None, index=True):
    """nn_plan -> nn_init -> nn_search -> nn_finalize.  qo / ro: int64 offsets [n_sets + 1] (default one set); rchunk: refs per work
    item (a multiple of kNnTile; 0 = the plan's own); q_begin / q_end narrow the query range the call writes.
    -> dict(dist, index, keys uint64 [n], prefix int64 [n_sets + 1], plan)"""
    L = lib()
    q, r = _c(q, np.float32).reshape(-1, 3), _c(r, np.float32).reshape(-1, 3)
    qo = _offsets(None, len(q)) if qo is None else _c(qo, np.int64)
    ro = _offsets(None, len(r)) if ro is None else _c(ro, np.int64)
    n_sets = len(qo) - 1
    plan = _ll(0, 0, 0, 0, 0)
    assert L.vmsim_nn_plan(_vp(qo), _vp(ro), n_sets, ctypes.c_longlong(len(q)), ctypes.c_longlong(rchunk), plan) == 0
    if q_begin is not None:
        plan[1] = int(q_begin)
    if q_end is not None:
        plan[2] = int(q_end)
    lay = _ll(0, 0)
    L.vmsim_nn_layout(ctypes.c_longlong(len(q)), n_sets, lay)
    ws, dist = _Buf(lay[1], np.uint8), _Buf(len(q), np.float32)
    idx = _Buf(len(q), np.int32) if index else None
    assert L.vmsim_nn(plan, _vp(q), _vp(qo), _vp(r), _vp(ro), n_sets, dist.ptr, idx.ptr if idx else None, ws.ptr) == 0
    ws.check_sections([(0, 8 * (n_sets + 1)), (lay[0], 8 * len(q))], "nn workspace"), dist.check("nn dist")
    if idx:
        idx.check("nn index")
    return dict(dist=dist.a, index=idx.a if idx else None, keys=ws.a[lay[0]:lay[0] + 8 * len(q)].view(np.uint64),
                prefix=ws.a[:8 * (n_sets + 1)].view(np.int64), plan=list(plan))


def sim_surface_sample(v, f, fo=None, oo=None, n_out=None, u0=None, r=None, seed=0, stream_id=0, set_base=0, o_begin=None, o_end=None,
                       face_index=True):
    """surface_cdf -> surface_sample.  fo / oo: int64 offsets of the faces / output points of each set.  u0 float64 [N] and r float32
    [N,2]: test mode; neither: Philox mode.  -> dict(points [N,3], face_index [N], cdf float64 [F])"""
    L = lib()
    v, f = _c(v, np.float32).reshape(-1, 3), _c(f, np.int32).reshape(-1, 3)
    fo = _offsets(None, len(f)) if fo is None else _c(fo, np.int64)
    oo = _offsets(None, n_out if n_out is not None else len(u0)) if oo is None else _c(oo, np.int64)
    N, n_sets = int(oo[-1]), len(fo) - 1
    u0c = _c(u0, np.float64) if u0 is not None else None
    rc = _c(r, np.float32) if r is not None else None
    ob, oe = oo[0] if o_begin is None else o_begin, oo[-1] if o_end is None else o_end
    L.vmsim_surface_sample_bytes.restype = ctypes.c_longlong
    ws = _Buf(L.vmsim_surface_sample_bytes(ctypes.c_longlong(len(f))), np.uint8)
    pts = _Buf((N, 3), np.float32)
    fi = _Buf(N, np.int32) if face_index else None
    assert L.vmsim_surface_sample(_vp(v), ctypes.c_longlong(len(v)), _vp(f), _vp(fo), _vp(oo), n_sets, ctypes.c_longlong(int(ob)),
                                  ctypes.c_longlong(int(oe)), ctypes.c_ulonglong(seed), ctypes.c_uint(stream_id), int(set_base), _vp(u0c),
                                  _vp(rc), pts.ptr, fi.ptr if fi else None, ws.ptr) == 0
    ws.check_sections([(0, 8 * len(f))], "cdf workspace"), pts.check("sample points")
    if fi:
        fi.check("sample faces")
    return dict(points=pts.a, face_index=fi.a if fi else None, cdf=ws.a[:8 * len(f)].view(np.float64))


def box15(center, R, extent):
    return np.concatenate([np.asarray(center, np.float32).ravel(), np.asarray(R, np.float32).ravel(), np.asarray(extent, np.float32).ravel()])


def sim_clip(v, f, box, cap=None):
    """clip_count -> clip_scan -> clip_emit.  box: float32 [15] = centre, row-major R (columns = axes), full extent; cap: triangle
    capacity (default the count).  -> dict(count, triangles [cap,3,3], blk int64 [nblk] exclusive prefix)"""
    L = lib()
    L.vmsim_clip_box_bytes.restype = ctypes.c_longlong
    v, f, box = _c(v, np.float32).reshape(-1, 3), _c(f, np.int32).reshape(-1, 3), _c(box, np.float32)
    ws, count = _Buf(L.vmsim_clip_box_bytes(ctypes.c_longlong(len(f))), np.uint8), _Buf(1, np.int64)
    assert L.vmsim_clip_count(_vp(v), ctypes.c_longlong(len(v)), _vp(f), ctypes.c_longlong(len(f)), _vp(box), count.ptr, ws.ptr) == 0
    nblk = (len(f) + 255) // 256
    ws.check_sections([(0, 8 * nblk)], "clip workspace after count"), count.check("clip count")
    total = int(count.a[0])
    cap = total if cap is None else int(cap)
    tri = _Buf((cap, 3, 3), np.float32)
    assert L.vmsim_clip_emit(_vp(v), ctypes.c_longlong(len(v)), _vp(f), ctypes.c_longlong(len(f)), _vp(box), tri.ptr, ctypes.c_longlong(cap),
                             ws.ptr) == 0
    ws.check_sections([(0, 8 * nblk)], "clip workspace"), tri.check("clip triangles")
    return dict(count=total, triangles=tri.a, blk=ws.a[:8 * nblk].view(np.int64))


def sim_unproject(depth, inst, t_wc, k4, pairs, first_pair, cap=None):
    """unproject_init -> _count -> _scan -> _emit.  depth float32 / inst int32 [n_slots,W,H], t_wc [n_slots,4,4], pairs int32
    [n_pairs,2] = (slot, instance id), first_pair int32 [n_obj + 1].  -> dict(offsets int64 [n_obj+1], bounds [n_obj,6], points [cap,3],
    blk int64 [n_pairs * nb] exclusive prefix)"""
    L = lib()
    depth, inst, t_wc = _c(depth, np.float32), _c(inst, np.int32), _c(t_wc, np.float32)
    n_slots, W, H = depth.shape
    pairs, first_pair = _c(pairs, np.int32).reshape(-1, 2), _c(first_pair, np.int32)
    n_pairs, n_obj = len(pairs), len(first_pair) - 1
    intr = _c(k4, np.float32)
    lay = _ll(0, 0, 0)
    L.vmsim_unproject_layout(n_pairs, n_obj, W, H, lay)
    ws, off, bnd = _Buf(lay[2], np.uint8), _Buf(n_obj + 1, np.int64), _Buf((n_obj, 6), np.float32)
    assert L.vmsim_unproject_count(_vp(depth), _vp(inst), _vp(t_wc), n_slots, W, H, _vp(intr), _vp(pairs), _vp(first_pair), n_obj, n_pairs,
                                   off.ptr, bnd.ptr, ws.ptr) == 0
    sections = [(0, 8 * n_pairs * lay[0]), (lay[1], 24 * n_obj)]
    ws.check_sections(sections, "unproject workspace after count"), off.check("offsets"), bnd.check("bounds")
    total = int(off.a[-1])
    cap = total if cap is None else int(cap)
    pts = _Buf((cap, 3), np.float32)
    assert L.vmsim_unproject_emit(_vp(depth), _vp(inst), _vp(t_wc), n_slots, W, H, _vp(intr), _vp(pairs), _vp(first_pair), n_obj, n_pairs,
                                  pts.ptr, ctypes.c_longlong(cap), ws.ptr) == 0
    ws.check_sections(sections, "unproject workspace"), pts.check("unprojected points")
    return dict(offsets=off.a, bounds=bnd.a, points=pts.a, blk=ws.a[:8 * n_pairs * lay[0]].view(np.int64), nb=lay[0])


def sim_obb_extents(points, po, rot, center=None, chunks=0):
    """obb_init -> obb_extents -> obb_decode.  rot: [K,3,3] shared by all objects or [n_obj,K,3,3]; chunks 0 = the automatic count.
    -> (lo, hi) float32 [n_obj,K,3]"""
    L = lib()
    p, po, rot = _c(points, np.float32).reshape(-1, 3), _c(po, np.int64), _c(rot, np.float32)
    n_obj = len(po) - 1
    K = rot.shape[-3]
    stride = 0 if rot.ndim == 3 else K * 9
    c = _c(center, np.float32) if center is not None else None
    if not chunks:
        chunks = L.vmsim_obb_chunks(_vp(po), n_obj, K)
    lo, hi = _Buf((n_obj, K, 3), np.float32), _Buf((n_obj, K, 3), np.float32)
    assert L.vmsim_obb_extents(_vp(p), _vp(po), n_obj, _vp(c), _vp(rot), ctypes.c_longlong(stride), K, int(chunks), lo.ptr, hi.ptr) == 0
    lo.check("obb lo"), hi.check("obb hi")
    return lo.a, hi.a


def sim_cloud_moments(points, po, center=None):
    """-> float64 [n_obj,9]: sums of (x, y, z, xx, xy, xz, yy, yz, zz) of the centred points"""
    p, po = _c(points, np.float32).reshape(-1, 3), _c(po, np.int64)
    c = _c(center, np.float32) if center is not None else None
    out = _Buf((len(po) - 1, 9), np.float64)
    assert lib().vmsim_cloud_moments(_vp(p), _vp(po), len(po) - 1, _vp(c), out.ptr) == 0
    out.check("moments")
    return out.a


def sim_enc_dec(x):
    """enc_f32 / dec_f32 of bounds_kernels.h, value by value -> (enc uint32, dec float32)"""
    x = _c(x, np.float32)
    enc, dec = _Buf(len(x), np.uint32), _Buf(len(x), np.float32)
    assert lib().vmsim_enc_dec(_vp(x), ctypes.c_longlong(len(x)), enc.ptr, dec.ptr) == 0
    enc.check("enc"), dec.check("dec")
    return enc.a, dec.a
