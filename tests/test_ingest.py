"""CPU tier of frame ingest: the numpy checker (tests/ingest_oracle.py) against the fixtures the reference's own loader produced
(tests/golden/make_ingest_goldens.py), the margin arithmetic against the torch expression the reference evaluates, csrc/ingest_rules.h -
compiled into the host program tests/tools/ingest_rules_host.cpp with the address and undefined-behaviour sanitizers - against the
checker, and the argument checks of vmapstep_ingest_* (no device is touched)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ingest_oracle as io
from conftest import ROOT, load_golden
from vmap_amd import _lib

FIXTURES = ("ingest_rects", "ingest_noise", "ingest_imap")
SCALES = (0.05, 0.2, 0.9, 1.0, 1.5)


def oracle_of(g, **kw):
    imap = bool(g["imap"])
    args = dict(background=g["background"].tolist(), bbox_scale=float(g["bbox_scale"]), min_box=int(g["min_box"]))
    args.update(kw)
    return io.ingest(g["rgb"], g["depth"], None if imap else g["inst"], None if imap else g["sem"], float(g["depth_scale"]), float(g["max_depth"]), **args)


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference_fixture(name):
    """obj, image, depth (bitwise), the boxes and the order of the ids: the checker against what dataset.Replica.__getitem__ returned."""
    g = load_golden(name)
    o = oracle_of(g)
    assert np.array_equal(o["inst"], g["ref_obj"]) and o["inst"].dtype == np.int32
    assert np.array_equal(o["rgbx"][..., :3], g["ref_image"]) and not o["rgbx"][..., 3].any()
    assert np.array_equal(o["depth"].view(np.uint32), g["ref_depth"].view(np.uint32))
    bd = io.bbox_dict(o["rows"])
    assert list(bd) == g["ref_bbox_ids"].tolist()                      # ascending, as np.unique walks them
    assert np.array_equal(np.asarray(list(bd.values()), np.int32).reshape(-1, 4), g["ref_bbox"])
    assert o["overflow"] == 0 and np.array_equal(o["rows"][:, 0], np.sort(o["rows"][:, 0]))


def test_fixtures_hold_the_cases_they_were_built_for():
    g = load_golden("ingest_rects")
    st = {int(r[0]): int(r[1]) for r in oracle_of(g)["rows"]}
    assert st == {0: io.BACKGROUND, 1: io.KEPT, 2: io.BACKGROUND, 3: io.SMALL, 4: io.KEPT, 5: io.KEPT, 6: io.KEPT, 300: io.KEPT}
    boxes = dict(zip(g["ref_bbox_ids"].tolist(), g["ref_bbox"].tolist()))
    assert boxes[5][1] == 63 and boxes[5][3] == 47 and boxes[0] == [0, 64, 0, 48]        # clipped at two borders; the full frame
    assert (g["ref_depth"] == 0).mean() > 0.1                                            # the depth filter acts
    n = oracle_of(load_golden("ingest_noise"))["rows"]
    assert len(n) >= 35 and {io.KEPT, io.BACKGROUND, io.SMALL} <= set(n[:, 1].tolist()) and n[:, 0].max() > 255
    assert oracle_of(load_golden("ingest_imap"))["rows"][:, 0].tolist() == [0] and not load_golden("ingest_imap")["ref_obj"].any()


def test_margin_equals_the_torch_expression_for_every_extent():
    """enlarge_bbox (utils.py:40-41) on the 0-dim int64 tensors get_bbox2d_batch returns: int(0.5 * scale * (max - min)), which torch
    computes in float32.  The contract's trunc(float32(0.5 * scale) * float32(extent)) for every extent an image can have."""
    lo = torch.tensor(3)
    for scale in SCALES:
        for e in range(4096):
            assert int(0.5 * scale * (torch.tensor(e + 3) - lo)) == io.margin(scale, e), (scale, e)


# ---- csrc/ingest_rules.h on the host ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, built with -fsanitize=address,undefined: any out-of-bounds access or undefined
    arithmetic in the rules aborts it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("ingest_host") / "ingest_rules_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "vmap_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "ingest_rules_host.cpp"), "-o", exe], check=True)
    return exe


def f32_bits(x):
    return f"{int(np.float32(x).view(np.uint32)):08x}"


def run_host(exe, tmp_path, lines):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    return subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]


def rule_line(W, H, scale, min_box, idv, stats):
    return f"R {W} {H} {f32_bits(np.float32(0.5 * scale))} {min_box} {idv} " + " ".join(str(int(s)) for s in stats)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_rules_equal_the_oracle_on_the_fixture_tables(host_exe, tmp_path, name):
    g = load_golden(name)
    H, W = g["inst"].shape
    imap = bool(g["imap"])
    table, _ = io.stats_table(np.zeros_like(g["inst"]) if imap else g["inst"], None if imap else g["sem"])
    bg, scale, mb = g["background"].tolist(), float(g["bbox_scale"]), int(g["min_box"])
    ids = sorted(table)
    out = run_host(host_exe, tmp_path, [f"B {len(bg)} " + " ".join(map(str, bg))] + [rule_line(W, H, scale, mb, i, table[i]) for i in ids])
    rows = oracle_of(g)["rows"]
    assert [[int(x) for x in l.split()] for l in out] == [[r[1], *r[3:7], r[7]] for r in rows.tolist()]


def test_host_rules_equal_the_oracle_on_random_rows(host_exe, tmp_path):
    """A few thousand random (extent, scale, min_box, class) rows: every status, clipping at every border, id 0 and id -1, absent
    rows; then the margin for every extent at every scale, the depth rule and the label rule."""
    rng = np.random.default_rng(7)
    bg = [5, 12, 40, 93, -1]
    lines, want = [f"B {len(bg)} " + " ".join(map(str, bg))], []
    for _ in range(4000):
        W, H = int(rng.integers(1, 4096)), int(rng.integers(1, 4096))
        scale = float(rng.choice(SCALES + (0.0, 0.3)))
        mb = int(rng.choice([-1, 0, 10, 25]))
        idv = int(rng.choice([-1, 0, 1, 7, 300, 65535]))
        eu, ev = (int(min(rng.choice([1, 2, 9, 10, 11, 12, 26, int(rng.integers(1, 4096))]), s)) for s in (W, H))
        u0, v0 = int(rng.integers(0, W - eu + 1)), int(rng.integers(0, H - ev + 1))
        c = int(rng.choice([-1, 0, 5, 7, 20, 93, 200]))
        c2 = c if rng.random() < 0.9 else c + int(rng.integers(1, 5))
        count = 0 if rng.random() < 0.05 else int(rng.integers(1, eu * ev + 1))
        stats = (count, u0, u0 + eu - 1, v0, v0 + ev - 1, c, c2)
        lines.append(rule_line(W, H, scale, mb, idv, stats))
        st, box, cls = io.decide(idv, stats, W, H, scale, mb, bg)
        want.append(f"{st} {box[0]} {box[1]} {box[2]} {box[3]} {cls}")
    for scale in SCALES:
        for e in range(4096):
            lines.append(f"M {f32_bits(np.float32(0.5 * scale))} {e}")
            want.append(str(io.margin(scale, e)))
    raws = np.concatenate([rng.integers(0, 65536, 500).astype(np.float32), (rng.random(500) * 12).astype(np.float32),
                           np.array([0.0, 8.0, np.nextafter(np.float32(8.0), np.float32(9.0)), np.inf, np.nan], np.float32)])
    for i, raw in enumerate(raws):
        sc, mx = (np.float32(1.0 / 6553.5), np.float32(8.0)) if i < 500 else (np.float32(1.0), np.float32(8.0))
        lines.append(f"D {f32_bits(raw)} {f32_bits(sc)} {f32_bits(mx)}")
        want.append(f32_bits(io.depth_of(np.array([raw]), sc, mx)[0]))
    for idv in (-1, 0, 5, 300):
        for st in range(6):
            lines.append(f"L {idv} {st}")
            want.append(str(idv if st == io.KEPT else 0))
    got = run_host(host_exe, tmp_path, lines)
    assert len(got) == len(want)
    bad = [(l, g, w) for l, g, w in zip(lines[1:], got, want) if g != w]
    assert not bad, bad[:5]
    assert {w.split()[0] for w in want[:4000]} == {str(s) for s in range(6)}                # every status occurred


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

def _cfg(width=64, height=48, max_ids=1024, n_background=2):
    bg = (ctypes.c_int32 * 64)(5, 12)
    return _lib.IngestCfg(width, height, 0, 0, 1.0 / 6553.5, 8.0, 0.2, 10, max_ids, n_background, bg)


def _call(lib, cfg, ws_bytes=None, rgb=True, sem=True, inst=True):
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    need = ctypes.c_size_t()
    if ws_bytes is None:
        assert lib.vmapstep_ingest_workspace_bytes(1024, ctypes.byref(need)) == 0
        ws_bytes = need.value
    return lib.vmapstep_ingest_frame(ctypes.byref(cfg) if cfg is not None else None, p if rgb else None, p, p if inst else None, p if sem else None,
                                     p, p, p, p, p, ws_bytes, None)


def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """One call per return code, none of which reads a pointer or touches a device: VMAPSTEP_ERR_ARGUMENT (-1) for null or
    inconsistent arguments, VMAPSTEP_ERR_UNSUPPORTED (-2) past a limit, VMAPSTEP_ERR_WORKSPACE (-3) for a short workspace - which is
    also as far as a well-formed call gets here."""
    lib = _lib.load()
    n = ctypes.c_size_t()
    assert lib.vmapstep_ingest_workspace_bytes(1024, ctypes.byref(n)) == 0 and n.value >= 1024 * 9 * 4
    small = n.value
    assert lib.vmapstep_ingest_workspace_bytes(65537, ctypes.byref(n)) == 0 and n.value > small
    assert lib.vmapstep_ingest_workspace_bytes(1024, None) == -1
    for bad in (1, 0, -5, 65538):
        assert lib.vmapstep_ingest_workspace_bytes(bad, ctypes.byref(n)) == -2 and b"max_ids" in lib.vmapstep_last_error()
    assert _call(lib, None) == -1 and b"cfg" in lib.vmapstep_last_error()
    assert _call(lib, _cfg(), rgb=False) == -1 and b"null" in lib.vmapstep_last_error()
    assert _call(lib, _cfg(), inst=False) == -1 and b"sem without inst" in lib.vmapstep_last_error()
    assert _call(lib, _cfg(width=0)) == -1
    assert _call(lib, _cfg(n_background=-1)) == -1
    for kw in (dict(width=4096), dict(height=4096), dict(max_ids=1), dict(max_ids=65538), dict(n_background=65)):
        assert _call(lib, _cfg(**kw)) == -2 and b"ingest limits" in lib.vmapstep_last_error(), kw
    assert _call(lib, _cfg(), ws_bytes=small - 1) == -3 and b"ingest workspace" in lib.vmapstep_last_error()
    assert _call(lib, _cfg(width=4095, height=4095, n_background=64, max_ids=65537), ws_bytes=0) == -3      # at every limit: passes them


def test_ingest_cfg_layout_matches_the_header(tmp_path):
    """The ctypes mirror of vmapstep_ingest_cfg against include/vmapstep.h as gcc lays it out: size and the offset of every field."""
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    fields = [f for f, _ in _lib.IngestCfg._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmapstep.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(vmapstep_ingest_cfg));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(vmapstep_ingest_cfg, {f}));\n' for f in fields)
                   + '  printf("classes %d\\n", VMAPSTEP_INGEST_MAX_CLASSES);\n  printf("status %d %d %d %d %d %d\\n", VMAPSTEP_INGEST_ABSENT, '
                   "VMAPSTEP_INGEST_KEPT, VMAPSTEP_INGEST_BACKGROUND, VMAPSTEP_INGEST_SMALL, VMAPSTEP_INGEST_ZERO_MARGIN, VMAPSTEP_INGEST_MIXED);\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(got["size"][0]) == ctypes.sizeof(_lib.IngestCfg)
    for f in fields:
        assert int(got[f][0]) == getattr(_lib.IngestCfg, f).offset, f
    assert int(got["classes"][0]) == _lib.INGEST_MAX_CLASSES
    assert [int(x) for x in got["status"]] == [io.ABSENT, io.KEPT, io.BACKGROUND, io.SMALL, io.ZERO_MARGIN, io.MIXED] == list(range(6))


def test_frame_ingest_refuses_a_cpu_store():
    from vmap_amd import ingest, keyframes
    store = keyframes.FrameStore(2, 16, 12, device="cpu")
    with pytest.raises(_lib.VmapStepError):
        ingest.FrameIngest(store, 1.0, 8.0)
    assert ingest.REPLICA_BACKGROUND_CLASSES == tuple(load_golden("ingest_rects")["background"].tolist())
    assert (ingest.KEPT, ingest.MIXED) == (io.KEPT, io.MIXED)


def test_free_slot_is_the_slot_put_takes():
    """FrameStore.free_slot, factored out of put for FrameIngest: the same choice, and put's behaviour unchanged."""
    from vmap_amd import keyframes
    st = keyframes.FrameStore(3, 4, 3, device="cpu")
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    frame = (z(4, 3, 3, dt=torch.uint8), z(4, 3), z(4, 3, dt=torch.int32), torch.eye(4))
    assert st.free_slot() == 0 and st.put(*frame, 10) == 0
    assert st.free_slot() == 1 and st.put(*frame, 11) == 1          # slot 0 waits for its retain
    st.retain(1)
    st.collect()
    assert st.free_slot() == 0 and st.put(*frame, 12) == 0 and st.put(*frame, 13) == 2
    with pytest.raises(RuntimeError):
        st.free_slot()
