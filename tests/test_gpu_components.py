"""GPU tier of mesh components (vmap_amd/components.py; csrc/component_kernels.h), through the C ABI and the Python API: labels,
counts and area_q equal the numpy checker (tests/components_oracle.py) exactly - everything is an integer, there is no tolerance
anywhere.  The shapes are the smallest at which the kernels can still go wrong: a strip over several workgroups in three numberings
(the longest parent chains), a fan around one hub (the most contention on one root and one statistics row), disjoint pieces with C
and V on both sides of every block and chunk edge (read from csrc/launch_geometry.h), random triples from many small pieces to one
giant one, and marching cubes of the committed volumes."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import components_cases as kc
import components_oracle as ko
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCK, SCAN, STATS = kc.geometry("kCompWG"), kc.geometry("kCompScanWG"), kc.geometry("kStatsWG")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def mesh_of(v, f, normals=None, colors=None):
    from vmap_amd import meshing
    return meshing.Mesh(dev(v), dev(f), None if normals is None else dev(normals), None if colors is None else dev(colors))


def check(v, f, areas=True):
    """label_components and component_stats against the checker; returns (labels, C) of the checker."""
    from vmap_amd import components
    want, C = ko.label(f, len(v))
    mesh = mesh_of(v, f)
    labels, n = components.label_components(mesh)
    assert labels.dtype == torch.int32 and labels.device == torch.device(DEV) and labels.shape == (len(v),)
    assert n == C and np.array_equal(labels.cpu().numpy(), want)
    nv, nf, aq = ko.stats(v if areas else None, f, want, C)
    st = components.component_stats(mesh, labels, n, areas=areas)
    assert st.vertices.dtype == torch.int32 and st.faces.dtype == torch.int64 and st.area_q.dtype == torch.int64 and len(st) == C
    assert np.array_equal(st.vertices.cpu().numpy(), nv) and np.array_equal(st.faces.cpu().numpy(), nf)
    assert np.array_equal(st.area_q.cpu().numpy(), aq)
    assert np.array_equal(st.area.cpu().numpy(), aq.astype(np.float64) * 2.0 ** -40)
    return want, C


def test_hand_made_mesh_with_its_answers_written_out():
    """Two tetrahedra, an unreferenced vertex, a face with a repeated index, two faces out of range (tests/components_cases.py)."""
    from vmap_amd import components
    v, f = kc.hand_made()
    labels, C = components.label_components(mesh_of(v, f))
    st = components.component_stats(mesh_of(v, f), labels, C)
    assert labels.tolist() == kc.HAND_LABELS and C == 4
    assert st.vertices.tolist() == kc.HAND_VERTICES and st.faces.tolist() == kc.HAND_FACES and st.area_q.tolist() == kc.HAND_AREA_Q
    assert components.component_stats(mesh_of(v, f), labels, C, areas=False).area_q.tolist() == [0, 0, 0, 0]
    check(v, f)


def test_area_edge_cases_on_the_device():
    """Halves in both directions, zero area, NaN / infinite coordinates, the clamp: see tests/test_components.py::test_area_edge_cases."""
    from vmap_amd import components
    v, f, want = kc.area_edge_cases()
    labels, C = components.label_components(mesh_of(v, f))
    assert C == len(f) and components.component_stats(mesh_of(v, f), labels, C).area_q.tolist() == want


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_strip_of_2000_faces(order):
    v, f = kc.strip(2000, order, seed=3)
    assert len(f) > 4 * BLOCK                                     # several workgroups hook the one component
    _, C = check(v, f)
    assert C == 1


@pytest.mark.parametrize("hub_high", [True, False])
def test_fan_of_5000_faces(hub_high):
    v, f = kc.fan(5000, hub_high)
    assert len(f) > 4 * STATS
    _, C = check(v, f)
    assert C == 1


def _edges():
    """(triangles, extra unreferenced vertices): V = 3 * triangles + extra and C = triangles + extra on both sides of one block of
    vertices (comp_flatten / comp_root_emit: BLOCK), one workgroup of the statistics (STATS) and one chunk of the block-total scan
    (SCAN blocks of BLOCK vertices); the empty mesh and the one-face mesh."""
    out = [(0, 0), (1, 0), (0, 1)]
    for edge in (BLOCK, STATS, BLOCK * SCAN):
        for n in (edge - 1, edge, edge + 1):
            out.append((n // 3, n % 3))                            # V = n
            if edge < BLOCK * SCAN:
                out.append((n, 0))                                 # C = F = n
    out.append((BLOCK * SCAN // 3 + 1, 0))                         # C one chunk of blocks' worth and more: V = 3 C spans > SCAN blocks
    return sorted(set(out))


@pytest.mark.parametrize("triangles,extra", _edges())
def test_disjoint_triangles_around_every_block_and_chunk_edge(triangles, extra):
    v, f = kc.disjoint_triangles(triangles, extra, seed=triangles)
    want, C = check(v, f)
    assert C == triangles + extra and len(v) == 3 * triangles + extra
    if len(v) > BLOCK * SCAN:
        assert -(-len(v) // BLOCK) > SCAN                         # more blocks than one chunk of comp_scan


@pytest.mark.parametrize("count", [1, BLOCK // 4, BLOCK // 4 + 1, STATS // 4 + 1, 3000])
def test_disjoint_tetrahedra(count):
    v, f = kc.disjoint_tetrahedra(count, seed=count)
    _, C = check(v, f)
    assert C == count


@pytest.mark.parametrize("F", [1000, 4000, 20000])
def test_random_triples_and_a_renumbering(F):
    """From many small pieces (F = 1000) to one giant piece (20 000).  The partition is invariant under a random renumbering of the
    vertices (compared as sets); labelling the same input a second time gives equal bytes."""
    from vmap_amd import components
    nv = 5000
    v, f = kc.random_triples(nv, F, seed=F)
    want, C = check(v, f)
    assert {1000: C > 1500, 4000: 50 < C < 1500, 20000: C < 10}[F], C
    perm = np.random.default_rng(F + 1).permutation(nv)
    v2, f2 = kc.renumber(v, f, perm)
    labels2, C2 = components.label_components(mesh_of(v2, f2))
    assert C2 == C
    assert ko.partition(labels2.cpu().numpy()[perm]) == ko.partition(want)       # vertex i of the original is perm[i] there
    again, C3 = components.label_components(mesh_of(v, f))                        # one extra run, not a loop
    assert C3 == C and again.cpu().numpy().tobytes() == want.tobytes()


def test_bad_indices_are_never_followed():
    v, f = kc.random_triples(3000, 5000, seed=9)
    f[::17, 1] = 3000
    f[5::23, 2] = -2
    f[7::29, 0] = np.iinfo(np.int32).max
    f[3::19, 0] = f[3::19, 1]
    check(v, f)


@pytest.mark.parametrize("name", ["mesh_blob", "mesh_noise", "white_noise"])
def test_marching_cubes_of_the_committed_volumes(name):
    """extract_mesh on the device, then labels and statistics against the checker.  The committed blob is one component, the
    committed (smooth) noise five, of 4 to 17 542 faces; a 24^3 volume of white noise made here adds hundreds of every size."""
    from vmap_amd import components, meshing
    vol = np.random.default_rng(5).random((24, 24, 24), np.float32) if name == "white_noise" else load_golden(name)["volume"]
    mesh = meshing.extract_mesh(dev(vol), 0.5)
    v, f = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
    want, C = ko.label(f, len(v))
    labels, n = components.label_components(mesh)
    assert n == C and np.array_equal(labels.cpu().numpy(), want)
    nv, nf, aq = ko.stats(v, f, want, C)
    st = components.component_stats(mesh, labels, n)
    assert np.array_equal(st.vertices.cpu().numpy(), nv) and np.array_equal(st.faces.cpu().numpy(), nf) and np.array_equal(st.area_q.cpu().numpy(), aq)
    print(f"{name}: {len(v)} vertices, {len(f)} faces, {C} components, faces per component {nf.min()} .. {nf.max()}")
    assert {"mesh_blob": C == 1, "mesh_noise": C >= 2, "white_noise": C >= 100}[name], C
    assert nf.sum() == len(f) and nv.sum() == len(v)


def test_keep_components():
    """Thresholds met with equality are kept; a largest=k tie goes to the lower number; largest beyond C; None when nothing is
    left; normals and colours travel; the kept mesh's own labels are dense again and its statistics are the kept rows."""
    from vmap_amd import components
    v, f = kc.hand_made()
    rng = np.random.default_rng(0)
    nrm = rng.standard_normal((len(v), 3)).astype(np.float32)
    col = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    mesh = mesh_of(v, f, nrm, col)
    unit = kc.HAND_AREA_Q[0]

    def kept_vertices(**kw):
        out = components.keep_components(mesh, **kw)
        want_f, want_k = ko.keep_components(v, f, **kw)[:2]
        if out is None:
            assert len(want_f) == 0
            return None
        assert np.array_equal(out.faces.cpu().numpy(), want_f) and np.array_equal(out.vertices.cpu().numpy(), v[want_k])
        assert np.array_equal(out.vertex_normals.cpu().numpy(), nrm[want_k]) and np.array_equal(out.vertex_colors.cpu().numpy(), col[want_k])
        return want_k.tolist()

    A, B, pair = [0, 1, 2, 3], [5, 6, 7, 8], [9, 10]
    assert kept_vertices() == A + B + pair                        # everything with a face; vertex 4 has none and goes
    assert kept_vertices(min_faces=4) == A + B and kept_vertices(min_faces=5) is None
    assert kept_vertices(min_area=unit * 2.0 ** -40) == A + B     # equality keeps
    assert kept_vertices(min_area=(unit + 1) * 2.0 ** -40) == B   # one unit more does not
    assert kept_vertices(min_area=(4 * unit + 1) * 2.0 ** -40) is None
    assert kept_vertices(largest=1) == B and kept_vertices(largest=2) == A + B
    assert kept_vertices(largest=3) == A + B                      # components 1 and 3 tie at area 0: the lower number (no face) wins the place
    assert kept_vertices(largest=4) == A + B + pair and kept_vertices(largest=99) == A + B + pair
    assert kept_vertices(largest=0) is None
    assert kept_vertices(largest=2, min_faces=1, min_area=(unit + 1) * 2.0 ** -40) == B

    # two components of exactly equal area: largest=1 keeps the lower number
    tv, tf = kc.disjoint_triangles(2)
    tv[:3] = np.round(tv[:3] * 8) / 8                             # coordinates on a grid: the translation changes no rounding
    tv[3:] = tv[:3] + np.float32(4.0)
    out, st = components.keep_components(mesh_of(tv, tf), largest=1, return_stats=True)
    assert st.area_q[0] == st.area_q[1] > 0 and st.kept.tolist() == [True, False] and out.faces.tolist() == [[0, 1, 2]]

    # a mesh with hundreds of components: the kept mesh relabelled is dense again and its statistics are the kept rows
    nv, F = 5000, 2000
    rv, rf = kc.random_triples(nv, F, seed=F)
    big = mesh_of(rv, rf)
    kw = dict(min_faces=2, min_area=0.2)
    out, st = components.keep_components(big, return_stats=True, **kw)
    want_f, want_k, _, C, (wnv, wnf, waq), keep = ko.keep_components(rv, rf, **kw)
    assert len(st) == C and np.array_equal(st.kept.cpu().numpy(), keep) and 1 < keep.sum() < C
    assert np.array_equal(out.faces.cpu().numpy(), want_f) and np.array_equal(out.vertices.cpu().numpy(), rv[want_k])
    labels, n = components.label_components(out)
    assert n == keep.sum() and labels.max() == n - 1
    st2 = components.component_stats(out, labels, n)
    assert np.array_equal(st2.vertices.cpu().numpy(), wnv[keep]) and np.array_equal(st2.faces.cpu().numpy(), wnf[keep])
    assert np.array_equal(st2.area_q.cpu().numpy(), waq[keep])


def test_weld_vertices():
    """A welded (indexed) mesh comes back unchanged; the separate triangles of crop_to_box, with a box holding everything, weld
    back to the original component count; -0.0 merges with +0.0; attributes are the first occurrence's."""
    from vmap_amd import components, evaluation, meshing
    mesh = meshing.extract_mesh(dev(load_golden("mesh_noise")["volume"]), 0.5)
    _, C = components.label_components(mesh)
    same = components.weld_vertices(mesh)
    assert torch.equal(same.vertices, mesh.vertices) and torch.equal(same.faces, mesh.faces) and torch.equal(same.vertex_normals, mesh.vertex_normals)
    soup = evaluation.crop_to_box(mesh, meshing.BoundingBox(center=[14, 14, 14], extent=[100, 100, 100]))
    assert len(soup.faces) == len(mesh.faces) and len(soup.vertices) == 3 * len(mesh.faces)
    assert components.label_components(soup)[1] == len(mesh.faces)           # one component per triangle
    welded = components.weld_vertices(soup)
    # marching-cubes vertices are distinct positions, every one referenced: welding finds exactly them
    assert len(welded.vertices) == len(mesh.vertices) and components.label_components(welded)[1] == C
    assert torch.equal(welded.vertices[welded.faces.long()], mesh.vertices[mesh.faces.long()])
    again = components.weld_vertices(welded)
    assert torch.equal(again.vertices, welded.vertices) and torch.equal(again.faces, welded.faces)       # idempotent
    # first occurrences in their order, attributes from the first occurrence, -0.0 == +0.0, different NaN-free bits stay apart
    v = np.array([[1, 2, 3], [0.0, 5, 6], [1, 2, 3], [-0.0, 5, 6], [7, 8, 9], [1, 2, np.nextafter(np.float32(3), np.float32(4))]], np.float32)
    col = np.arange(18, dtype=np.uint8).reshape(6, 3)
    f = np.array([[0, 1, 4], [2, 3, 5], [3, 9, 0]], np.int32)
    w = components.weld_vertices(mesh_of(v, f, v + 1, col))
    assert np.array_equal(w.vertices.cpu().numpy().view(np.uint32), v[[0, 1, 4, 5]].view(np.uint32))
    assert w.faces.tolist() == [[0, 1, 2], [0, 1, 3], [-1, -1, -1]] and w.vertex_colors.tolist() == col[[0, 1, 4, 5]].tolist()
    assert np.array_equal(w.vertex_normals.cpu().numpy(), (v + 1)[[0, 1, 4, 5]])


def _trainer(seed=0):
    from vmap_amd import trainer
    torch.manual_seed(seed)
    cfg = trainer.SimpleConfig()
    cfg.training_device, cfg.hidden_feature_size, cfg.obj_id = DEV, 32, 1
    return trainer.Trainer(cfg)


def test_trainer_meshing_drops_floaters_before_the_colour_query():
    """A small synthetic field (hidden 32, grid 32).  Without the keywords the output is byte-identical to the plain call; with
    largest_components=1 it is one component, and its colours equal those of the unfiltered call at the same vertices."""
    from vmap_amd import components, meshing
    tr = _trainer()                                               # untrained: over a 3 m box its occupancy crosses 0.5 around dozens of blobs
    bound = meshing.BoundingBox(center=[0.1, -0.2, 0.3], extent=[3.0, 3.6, 2.4])
    centre = torch.tensor([0.1, -0.2, 0.3], device=DEV)
    plain = tr.meshing(bound, centre, grid_dim=32)
    assert plain is not None
    off = tr.meshing(bound, centre, grid_dim=32, min_component_area=None, largest_components=None)
    for a, b in ((plain.vertices, off.vertices), (plain.faces, off.faces), (plain.vertex_normals, off.vertex_normals), (plain.vertex_colors, off.vertex_colors)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    labels, C = components.label_components(plain)
    assert C > 1, "the synthetic field has one piece only: the test shows nothing"
    one = tr.meshing(bound, centre, grid_dim=32, largest_components=1)
    assert components.label_components(one)[1] == 1
    st = components.component_stats(plain, labels, C)
    big = int(torch.sort(st.area_q, descending=True, stable=True).indices[0])
    idx = (labels == big).nonzero().reshape(-1)
    assert torch.equal(one.vertices, plain.vertices[idx]) and torch.equal(one.vertex_colors, plain.vertex_colors[idx])
    assert torch.equal(one.vertex_normals, plain.vertex_normals[idx]) and len(one.faces) == int(st.faces[big])
    smallest = float(st.area[st.faces > 0].min())
    by_area = tr.meshing(bound, centre, grid_dim=32, min_component_area=smallest * 1.5)
    assert 1 <= components.label_components(by_area)[1] < C
    assert tr.meshing(bound, centre, grid_dim=32, min_component_area=1e9) is None


def _write_obj(path, vertices, faces):
    with open(path, "w") as fh:
        for p in vertices:
            fh.write(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n")
        for f in faces:
            fh.write(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}\n")


def _run_cli(argv):
    from vmap_amd import evaluation
    buf = io.StringIO()
    with redirect_stdout(buf):
        rc = evaluation.main(argv)
    return rc, buf.getvalue()


def test_cli_with_and_without_the_flags(tmp_path):
    """python -m vmap_amd.evaluation REC GT --largest-components 1 --min-component-area X: REC is a sphere plus two small floaters, GT
    the sphere in the other triangulation.  With the flags the result is calc_3d_metric's on the filtered REC and the JSON carries
    the component count before and after; without them the output is what it was before the options existed, byte for byte."""
    from vmap_amd import components, evaluation, meshing
    g = load_golden("mesh_sphere")
    sv, sf = g["lewiner_vertices"] * np.float32(0.01), g["lewiner_faces"]
    tv, tf = kc.disjoint_tetrahedra(2, seed=1)
    tv = tv * np.float32(0.01) + np.float32(0.6)
    rec, gt = str(tmp_path / "rec.obj"), str(tmp_path / "gt.obj")
    _write_obj(rec, np.concatenate([sv, tv]), np.concatenate([sf, tf + len(sv)]))
    _write_obj(gt, g["lorensen_vertices"] * np.float32(0.01), g["lorensen_faces"])
    rc0, out0 = _run_cli([rec, gt, "--n", "3000", "--seed", "5"])
    m0 = evaluation.calc_3d_metric(meshing.load_mesh(rec), meshing.load_mesh(gt), N=3000, seed=5)
    assert rc0 == 0 and out0 == json.dumps({"rec": rec, "gt": gt, "n": 3000, "seed": 5, "accuracy": m0[0][0], "completion": m0[1][0],
                                            "completion_ratio_1cm": m0[2][0], "completion_ratio_5cm": m0[3][0]}) + "\n"
    rc, out = _run_cli([rec, gt, "--n", "3000", "--seed", "5", "--largest-components", "1", "--min-component-area", "1e-4"])
    res = json.loads(out)
    assert rc == 0 and res["rec_components"] == 3 and res["rec_components_kept"] == 1
    assert res["largest_components"] == 1 and res["min_component_area"] == 1e-4
    filtered = components.keep_components(meshing.load_mesh(rec), min_area=1e-4, largest=1)
    assert len(filtered.faces) == len(sf)
    m = evaluation.calc_3d_metric(filtered, meshing.load_mesh(gt), N=3000, seed=5)
    assert [res["accuracy"], res["completion"], res["completion_ratio_1cm"], res["completion_ratio_5cm"]] == [x[0] for x in m]
    rc2, out2 = _run_cli([rec, gt, "--n", "3000", "--min-component-area", "1e9"])
    assert rc2 == 1 and json.loads(out2)["result"] is None and json.loads(out2)["rec_components_kept"] == 0
