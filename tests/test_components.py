"""CPU tier of mesh components: the numpy checker (tests/components_oracle.py) against scipy's connected_components - the one outside
implementation the feature can be held against -, csrc/component_rules.h compiled into the host program
tests/tools/component_rules_host.cpp (one thread under the address and undefined-behaviour sanitizers; four racing threads under the
thread sanitizer) against the checker bit for bit, the area's edge cases with their answers written out, and the argument checks of
vmapstep_components_* and of vmap_amd/components.py (no device is touched)."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import components_cases as kc
import components_oracle as ko
from conftest import ROOT
from vmap_amd import _lib


def cases():
    """name -> (vertices, faces): small versions of every shape of the GPU tier."""
    out = {"hand": kc.hand_made(), "empty": (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)),
           "one_face": kc.disjoint_triangles(1), "no_face": (kc.positions(5, 1), np.zeros((0, 3), np.int32)),
           "triangles": kc.disjoint_triangles(70, extra_vertices=3), "tetrahedra": kc.disjoint_tetrahedra(40),
           "fan_high": kc.fan(300, True), "fan_low": kc.fan(300, False)}
    for order in ("ascending", "descending", "random"):
        out["strip_" + order] = kc.strip(400, order, seed=2)
    for F in (100, 400, 2000):
        out[f"random_{F}"] = kc.random_triples(500, F, seed=F)
    v, f = kc.random_triples(300, 200, seed=9)
    f[::17, 1] = 300                                              # out of range
    f[5::23, 2] = -2
    f[3::19, 0] = f[3::19, 1]                                     # repeated
    out["random_bad_indices"] = (v, f)
    return out


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_checker_labels_equal_scipy(name):
    """scipy numbers the components in the order of their first vertex, as the contract does: the labels are equal, not merely the
    partition."""
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    v, f = CASES[name]
    n = len(v)
    labels, C = ko.label(f, n)
    if n == 0:
        assert C == 0 and len(labels) == 0
        return
    fv = np.asarray(f, np.int64)[ko.valid_faces(f, n)]
    rows, cols = np.concatenate([fv[:, 0], fv[:, 1]]), np.concatenate([fv[:, 1], fv[:, 2]])
    graph = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    want_c, want = connected_components(graph, directed=False)
    assert C == want_c and np.array_equal(labels, want)


def test_checker_on_the_hand_made_mesh():
    v, f = kc.hand_made()
    labels, C = ko.label(f, len(v))
    nv, nf, aq = ko.stats(v, f, labels, C)
    assert labels.tolist() == kc.HAND_LABELS and C == 4
    assert nv.tolist() == kc.HAND_VERTICES and nf.tolist() == kc.HAND_FACES and aq.tolist() == kc.HAND_AREA_Q
    assert ko.stats(None, f, labels, C)[2].tolist() == [0, 0, 0, 0]
    # selection: equality keeps; largest ties go to the lower number; largest beyond C keeps all
    assert ko.select(nf, aq, min_faces=4).tolist() == [True, False, True, False]
    assert ko.select(nf, aq, min_area=kc.HAND_AREA_Q[0] * 2.0 ** -40).tolist() == [True, False, True, False]
    assert ko.select(nf, aq, min_area=(kc.HAND_AREA_Q[0] + 1) * 2.0 ** -40).tolist() == [False, False, True, False]
    assert ko.select(nf, aq, largest=1).tolist() == [False, False, True, False]
    assert ko.select(nf, aq, largest=3).tolist() == [True, True, True, False]      # 1 and 3 tie at area 0: the lower number
    assert ko.select(nf, aq, largest=9).all() and not ko.select(nf, aq, largest=0).any()


# ---- the host programs -------------------------------------------------------------------------------------------------------------------

def _build(tmp_path_factory, name, flags):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off"] + flags + ["-I", os.path.join(ROOT, "vmap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "component_rules_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """A stand-alone program with its own main, -fsanitize=address,undefined: an index the rules should not have followed, or
    undefined arithmetic in them, aborts it."""
    return _build(tmp_path_factory, "component_rules_host", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


@pytest.fixture(scope="module")
def threads_exe(tmp_path_factory):
    """The same source as a second stand-alone program: four threads race through the same loops over __atomic builtins, under
    the thread sanitizer."""
    return _build(tmp_path_factory, "component_rules_threads", ["-DKR_THREADS=4", "-fsanitize=thread", "-pthread"])


def run_host(exe, tmp_path, vertices, faces, shortening=1, min_faces=0, min_area=0.0, largest=None):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bits = struct.unpack("<Q", struct.pack("<d", float(min_area)))[0]
    lines = [f"{len(v)} {len(f)} {shortening} {min_faces} {-1 if largest is None else largest}", f"{bits:x}",
             " ".join(str(x) for x in f.reshape(-1).tolist()), " ".join(f"{x:08x}" for x in v.reshape(-1).view(np.uint32).tolist())]
    path = tmp_path / "mesh.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], check=True, capture_output=True, text=True).stdout.split("\n")
    ints = lambda s: np.array([int(x) for x in s.split()], np.int64)
    return ints(out[0]).astype(np.int32), int(out[1]), ints(out[2]), ints(out[3]), ints(out[4]), np.array([c == "1" for c in out[5].strip()], bool)


def orders(faces, seed=0):
    f = np.asarray(faces).reshape(-1, 3)
    return {"given": f, "reversed": f[::-1], "shuffled": f[np.random.default_rng(seed).permutation(len(f))]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_program_equals_the_checker(host_exe, tmp_path, name):
    """Labels, counts, area_q and decisions bit for bit, whatever the order of the unions and with or without path shortening."""
    v, f = CASES[name]
    labels, C = ko.label(f, len(v))
    nv, nf, aq = ko.stats(v, f, labels, C)
    thresholds = dict(min_faces=1, min_area=float(np.median(aq)) * 2.0 ** -40 if C else 0.0, largest=max(1, C // 2))
    keep = ko.select(nf, aq, **thresholds)
    for order, faces in orders(f).items():
        for shortening in (0, 1):
            got = run_host(host_exe, tmp_path, v, faces, shortening, **thresholds)
            assert got[1] == C and np.array_equal(got[0], labels), (order, shortening)
            assert np.array_equal(got[2], nv) and np.array_equal(got[3], nf) and np.array_equal(got[4], aq), (order, shortening)
            assert np.array_equal(got[5], keep), (order, shortening)
    if C > 3 and nf.max() > 0:
        assert 0 < keep.sum() < C                                 # the thresholds decide something


@pytest.mark.parametrize("name", ["hand", "strip_ascending", "strip_descending", "strip_random", "fan_high", "fan_low", "random_400", "random_2000",
                                  "random_bad_indices", "tetrahedra"])
def test_four_racing_threads_give_the_same_labels(threads_exe, tmp_path, name):
    """The strip gives the longest chains, the fan the most contention on one root; a data race or a lost union would show as a
    thread-sanitizer report (a non-zero exit) or as other labels."""
    v, f = CASES[name]
    labels, C = ko.label(f, len(v))
    nv, nf, aq = ko.stats(v, f, labels, C)
    for order, faces in orders(f, seed=1).items():
        for shortening in (0, 1):
            got = run_host(threads_exe, tmp_path, v, faces, shortening)
            assert got[1] == C and np.array_equal(got[0], labels), (order, shortening)
            assert np.array_equal(got[2], nv) and np.array_equal(got[3], nf) and np.array_equal(got[4], aq)


def test_area_edge_cases(host_exe, tmp_path):
    """The quantisation lands on a half in both directions (0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4), a zero-area triangle, NaN and
    infinite coordinates and an area that overflows count 0, the clamp at 2^62 and the float32 just below it."""
    v, f, want = kc.area_edge_cases()
    area = ko.triangle_area_f32(v, f)
    assert ko.quantise_area(area).tolist() == want
    labels, C = ko.label(f, len(v))
    assert C == len(f) and ko.stats(v, f, labels, C)[2].tolist() == want
    got = run_host(host_exe, tmp_path, v, f)
    assert got[4].tolist() == want and got[1] == C
    assert np.isnan(area[10]) and np.isinf(area[9]) and area[13] == 0
    assert ko.quantise_area(np.array([-1.0, -0.0, np.nan, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 0, 0, 0]
    # the threshold of the keep decision rounds the same way
    assert [ko.area_threshold(x * 2.0 ** -40) for x in (0.5, 1.5, 2.5, 3.5, 0.0)] == [0, 2, 2, 4, 0] and ko.area_threshold(2.0 ** 30) == 1 << 62


# ---- the C ABI's and the Python layer's argument checks --------------------------------------------------------------------------------

def test_abi_refuses_bad_arguments_before_anything_is_enqueued():
    """VMAPSTEP_ERR_ARGUMENT (-1) with a message, a short or misaligned workspace -3; none of the calls reads a pointer or touches a
    device.  No struct was added: there is no layout to check."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(16384)
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 256
    ref = ctypes.byref
    n = ctypes.c_size_t()
    assert lib.vmapstep_components_workspace_bytes(100, 200, ref(n)) == 0 and n.value >= 2 * 400 + 8
    need = n.value
    assert lib.vmapstep_components_workspace_bytes(0, 0, ref(n)) == 0
    for nv, nf in ((-1, 5), (5, -1), (1 << 31, 5), (5, 1 << 31)):
        assert lib.vmapstep_components_workspace_bytes(nv, nf, ref(n)) == -1 and lib.vmapstep_last_error().startswith(b"components")
    assert lib.vmapstep_components_workspace_bytes(100, 200, None) == -1
    label = lambda faces=p, nf=200, nv=100, labels=p, counts=p, ws=p, nb=need: lib.vmapstep_components_label(faces, nf, nv, labels, counts, ws, nb, None)
    assert label(faces=None) == -1 and label(labels=None) == -1 and label(counts=None) == -1
    assert label(nf=-1) == -1 and label(nv=-1) == -1 and label(nv=1 << 31) == -1 and label(nf=1 << 31) == -1
    assert label(nb=need - 1) == -3 and label(ws=p + 8) == -3 and b"components workspace" in lib.vmapstep_last_error()
    stats = lambda vertices=p, faces=p, nf=200, labels=p, nv=100, C=7, cv=p, cf=p, ca=p: \
        lib.vmapstep_components_stats(vertices, faces, nf, labels, nv, C, cv, cf, ca, None)
    assert stats(faces=None) == -1 and stats(labels=None) == -1 and stats(cv=None) == -1 and stats(cf=None) == -1 and stats(ca=None) == -1
    assert stats(nf=-1) == -1 and stats(nv=-1) == -1 and stats(nv=1 << 31) == -1
    assert stats(C=-1) == -1 and stats(C=101) == -1 and b"n_components" in lib.vmapstep_last_error()
    # no row to write: OK, nothing enqueued, no pointer looked at
    assert stats(C=0, cv=None, cf=None, ca=None) == 0 and stats(nv=0, nf=0, C=0, faces=None, labels=None, vertices=None) == 0
    assert lib.vmapstep_abi_version() == 7
    assert all(e in _lib.EXPORTS for e in ("vmapstep_components_workspace_bytes", "vmapstep_components_label", "vmapstep_components_stats"))


def test_python_layer_refuses_what_it_can_before_the_library():
    import torch
    import vmap_amd
    from vmap_amd import components
    assert "components" in vmap_amd.__all__
    assert {"label_components", "component_stats", "keep_components", "weld_vertices", "ComponentStats"} <= set(components.__all__)
    for bad in (-1.0, float("nan")):
        with pytest.raises(_lib.VmapStepError):
            components.area_threshold(bad)
    assert [components.area_threshold(x * 2.0 ** -40) for x in (0.5, 1.5, 2.5, 3.5)] == [0, 2, 2, 4]
    assert components.area_threshold(1e30) == 1 << 62 and components.area_threshold(0.0) == 0
    st = components.ComponentStats(torch.tensor([4, 1, 4, 2], dtype=torch.int32), torch.tensor(kc.HAND_FACES), torch.tensor(kc.HAND_AREA_Q))
    assert st.area.dtype == torch.float64 and st.area[0].item() == kc.HAND_AREA_Q[0] * 2.0 ** -40 and len(st) == 4
    sel = lambda **kw: components.select_components(st, **kw).tolist()
    assert sel(min_faces=4) == [True, False, True, False] and sel(largest=1) == [False, False, True, False]
    assert sel(largest=3) == [True, True, True, False] and sel(largest=9) == [True] * 4 and sel(largest=0) == [False] * 4
    assert sel(min_area=kc.HAND_AREA_Q[0] * 2.0 ** -40) == [True, False, True, False]
    with pytest.raises(_lib.VmapStepError):
        components.select_components(st, min_faces=-1)
    with pytest.raises(_lib.VmapStepError):
        components.select_components(st, largest=-1)
