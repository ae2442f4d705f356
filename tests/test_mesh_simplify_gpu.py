"""Mesh simplification on the device (multiply_amd/simplify.py, csrc/simplify.hip) against the float64 statement of the algorithm
(tests/mesh_simplify_reference.py): cell ids and faces bit for bit, positions and attribute means within the bounds derived in
tests/tolerances_simplify.py, the same bits on a second run."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import mesh_simplify_reference as R
from tests import mesh_simplify_shapes as S
from tests import tolerances_simplify as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
LAM = 1e-3
COUNTS = ("n_cells", "n_collapsed", "n_duplicate", "n_unreferenced", "passes")


def on_device(v, f):
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(DEV), torch.from_numpy(np.ascontiguousarray(f, np.int64)).to(DEV)


def simplify(v, f, **kw):
    from multiply_amd.simplify import simplify_mesh
    out = simplify_mesh(*on_device(v, f), **kw)
    torch.cuda.synchronize()
    return out


def check(what, got, ref):
    """faces and counts equal, every position within its bound; prints the worst position against its bound"""
    verts, faces, info = got
    assert faces.dtype == torch.int64 and verts.dtype == torch.float32 and verts.is_cuda and faces.is_cuda
    assert {k: info[k] for k in COUNTS} == {k: ref["info"][k] for k in COUNTS}, (what, info, ref["info"])
    assert info["cell"] == ref["info"]["cell"] and np.array_equal(info["origin"], ref["info"]["origin"]), what
    assert np.array_equal(faces.cpu().numpy(), ref["faces"]), what
    assert tuple(verts.shape) == ref["verts64"].shape, what
    if verts.shape[0] == 0:
        return
    h = ref["info"]["cell"]
    bound = T.position_bound(np.abs(ref["verts64"]).max(), ref["seg"], ref["n_verts"], ref["reach"], h, LAM)
    err = np.abs(verts.cpu().numpy().astype(np.float64) - ref["verts64"]).max(1)
    k = int(np.argmax(err / bound))
    print(f"[simplify {what}] {faces.shape[0]} faces, {verts.shape[0]} vertices, longest segment {int(ref['seg'].max())}: "
          f"|position - float64| at most {err.max():.3e}, worst against its bound {err[k]:.3e} / {bound[k]:.3e} "
          f"(double part {T.double_part(ref['seg'][k], ref['n_verts'][k], ref['reach'][k], h, LAM):.1e})")
    assert (err <= bound).all(), (what, float(err[k]), float(bound[k]))


# ------------------------------------------------------------------------------------------------ 1. cells
@pytest.mark.parametrize("case", ["squashed", "lattice", "lattice, origin below"])
def test_cell_ids_are_exact(case):
    from multiply_amd import hip
    if case == "squashed":
        (v, f), h, lo = S.squashed(3), 0.11, None
    else:
        (v, f), h = S.lattice_sheet(0.125, 9), 0.125
        lo = None if case == "lattice" else v[0] - np.float32(3 * 0.125)
    lo = R.origin_of(v) if lo is None else np.asarray(lo, np.float32)
    keys, cell = R.cell_ids(v, h, lo)
    got = hip.simplify_keys(on_device(v, f)[0], lo, np.float32(1.0) / np.float32(h))
    got_keys, got_cell = torch.unique(got, return_inverse=True)
    assert np.array_equal(got.cpu().numpy(), keys[cell])                    # the key of every vertex, bit for bit
    assert np.array_equal(got_keys.cpu().numpy(), keys) and np.array_equal(got_cell.cpu().numpy(), cell)
    if case != "squashed":                                                  # every vertex ON a cell face: its own cell, no neighbour's
        assert keys.shape[0] == v.shape[0]
    from multiply_amd.simplify import cluster_counts
    assert cluster_counts(*on_device(v, f), h, origin=lo) == R.cluster_counts(v, f, h, lo)


# ------------------------------------------------------------------------------------------------ 2. the whole result
@pytest.fixture(scope="module")
def references():
    cases = {"squashed 0.11": (S.squashed(4), 0.11), "squashed 0.05": (S.squashed(4), 0.05), "sheet 0.3": (S.two_sided_sheet(), 0.3),
             "box 0.13": (S.tessellated_box(), 0.13), "box 0.6": (S.tessellated_box(), 0.6)}
    return {k: (v, f, h, R.simplify(v, f, h)) for k, ((v, f), h) in cases.items()}


@pytest.mark.parametrize("case", ["squashed 0.11", "squashed 0.05", "sheet 0.3", "box 0.13"])
def test_result_against_the_reference_and_run_to_run(references, case):
    v, f, h, ref = references[case]
    got = simplify(v, f, cell=h)
    check(case, got, ref)
    again = simplify(v, f, cell=h)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    if case == "sheet 0.3":
        assert got[2]["n_duplicate"] == 18 and got[1].shape[0] == 18
        assert np.array_equal(got[1].cpu().numpy(), ref["faces"])          # the lower sheet's winding: the lower face index wins


# ------------------------------------------------------------------------------------------------ 3. long and empty segments
def test_long_segments(references):
    from multiply_amd import hip
    v, f, h, ref = references["box 0.6"]
    assert ref["seg"].max() > 256 and ref["seg"].max() > 64 * hip.SIMPLIFY_LANES and ref["info"]["n_cells"] == 8
    got = simplify(v, f, cell=h)
    check("box 0.6", got, ref)
    again = simplify(v, f, cell=h)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])


def test_vertices_of_no_face_are_compacted_away():
    v, f = S.squashed(3)
    extra = np.array([[0.9, 0.9, 0.9], [0.9, 0.9, 0.901], [-0.9, 0.2, 0.1], [0.0, 0.0, 0.0], [0.4, -1.2, 0.3]], np.float32)
    v2 = np.concatenate([v[:100], extra[:2], v[100:], extra[2:]]).astype(np.float32)
    f2 = f + 2 * (f >= 100)
    h = 0.11
    ref = R.simplify(v2, f2, h)
    assert ref["info"]["n_unreferenced"] == 4                               # the two at 0.9 share a cell
    got = simplify(v2, f2, cell=h)
    check("squashed(3) with 5 loose vertices", got, ref)
    plain = simplify(v, f, cell=h, origin=R.origin_of(v2))                 # the same cells without them: the same mesh
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])


# ------------------------------------------------------------------------------------------------ 4. degenerate input
def test_no_faces_and_one_cell():
    v, f = S.squashed(2)
    verts, faces, info = simplify(v, np.zeros((0, 3), np.int64), cell=0.11)
    n_cells = R.cell_ids(v, 0.11)[0].shape[0]
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and faces.dtype == torch.int64
    assert (info["n_cells"], info["n_collapsed"], info["n_duplicate"], info["n_unreferenced"]) == (n_cells, 0, 0, n_cells)
    verts, faces, info = simplify(v, f, cell=4.0, attrs=np.ones((v.shape[0], 3), np.float32))
    assert tuple(verts.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(info["attrs"].shape) == (0, 3)
    assert (info["n_cells"], info["n_collapsed"], info["n_duplicate"], info["n_unreferenced"]) == (1, f.shape[0], 0, 1)
    check("one cell", (verts, faces, info), R.simplify(v, f, 4.0))
    verts, faces, info = simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), cell=0.5)
    assert verts.shape[0] == 0 and faces.shape[0] == 0 and info["n_cells"] == 0


def test_faces_that_repeat_a_vertex_add_exactly_nothing():
    v, f = S.squashed(3)
    rng = np.random.RandomState(0)
    i, j = rng.randint(0, v.shape[0], 40), rng.randint(0, v.shape[0], 40)
    f2 = np.concatenate([f[:300], np.stack([i, j, j], 1), np.stack([j, j, i], 1), np.stack([i, i, i], 1), f[300:]])
    h = 0.11
    ref = R.simplify(v, f2, h)
    assert ref["info"]["n_collapsed"] == R.simplify(v, f, h)["info"]["n_collapsed"] + 120
    got = simplify(v, f2, cell=h)
    check("squashed(3) with 120 faces that repeat a vertex", got, ref)
    plain = simplify(v, f, cell=h)                                          # n = 0 bit for bit: not one position moves
    assert torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])


def test_cells_with_zero_area_faces_only_take_the_mean():
    """collinear, axis-aligned points: every cross product is exactly 0, the faces span three cells each and stay"""
    v = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.05, 0, 0], [0.3, 0, 0], [0.55, 0, 0], [0, 0.25, 0], [0, 0.5, 0]], np.float32)
    f = np.array([[0, 1, 2], [3, 4, 5], [0, 6, 7], [2, 1, 0]], np.int64)
    h = 0.2
    ref = R.simplify(v, f, h)
    assert ref["faces"].shape[0] == 2 and ref["info"]["n_duplicate"] == 2 and ref["info"]["n_collapsed"] == 0
    assert np.array_equal(ref["verts64"], ref["mean64"]) and (ref["seg"] > 0).all()
    got = simplify(v, f, cell=h)
    check("collinear faces", got, ref)
    assert np.abs(got[0].cpu().numpy() - ref["mean64"]).max() <= T.half_ulp32(0.55) + 8 * T.U


def test_bad_input_raises_before_any_launch(monkeypatch):
    from multiply_amd import hip
    from multiply_amd.simplify import cluster_counts, simplify_mesh
    v, f = S.squashed(2)
    vt, ft = on_device(v, f)
    launched = []
    lib = hip.lib()
    for name in ("mp_simplify_keys", "mp_simplify_count", "mp_simplify_faces", "mp_simplify_first", "mp_simplify_quadrics",
                 "mp_simplify_attr_mean"):
        assert hasattr(lib, name)

    class Spy:
        def __getattr__(self, name):
            if name.startswith("mp_simplify"):
                launched.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(hip, "lib", lambda: Spy())
    for bad in (np.nan, np.inf, -np.inf):
        w = vt.clone()
        w[17, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            simplify_mesh(w, ft, cell=0.1)
        with pytest.raises(ValueError, match="finite"):
            simplify_mesh(w, ft, target_faces=100)
        with pytest.raises(ValueError, match="finite"):
            cluster_counts(w, ft, 0.1)
    with pytest.raises(ValueError, match="fit"):
        simplify_mesh(vt, ft, cell=1e-7)
    with pytest.raises(ValueError, match="fit"):
        simplify_mesh(vt, ft, cell=0.1, origin=[0.0, 0.0, 0.0])
    g = ft.clone()
    g[5, 2] = vt.shape[0]
    with pytest.raises(ValueError, match="outside"):
        simplify_mesh(vt, g, cell=0.1)
    with pytest.raises(ValueError, match="attrs"):
        simplify_mesh(vt, ft, cell=0.1, attrs=torch.zeros(3, 2))
    assert launched == []
    simplify_mesh(vt, ft, cell=0.1)
    assert "mp_simplify_quadrics" in launched


# ------------------------------------------------------------------------------------------------ 5. corners
def test_box_corners_on_the_device(references):
    v, f, h, ref = references["box 0.13"]
    verts, faces, _ = simplify(v, f, cell=h)
    out_v, out_f = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy()
    corners = S.box_corners()
    dq = np.sqrt(((corners[:, None] - out_v[None]) ** 2).sum(-1)).min(1) / h
    dm = np.sqrt(((corners[:, None] - ref["mean64"][None]) ** 2).sum(-1)).min(1) / h
    ratio = R.volume(out_v, out_f) / R.volume(v, f)
    print(f"[simplify box 0.13, device] corners within {dq.max():.2e} h of an output vertex (cell means: {dm.min():.2f} h); volume ratio {ratio:.6f}")
    assert dq.max() <= 0.01 and dm.min() >= 0.4 and R.is_watertight(out_f) and abs(ratio - 1.0) <= 1e-3


# ------------------------------------------------------------------------------------------------ 6. attributes
def test_attribute_means():
    v, f = S.squashed(4)
    rng = np.random.RandomState(5)
    w = rng.uniform(0, 1, (v.shape[0], 24)) ** 4
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    h = 0.11
    ref = R.simplify(v, f, h, attrs=w)
    verts, faces, info = simplify(v, f, cell=h, attrs=w)
    check("squashed 0.11 with attributes", (verts, faces, info), ref)
    got = info["attrs"].cpu().numpy().astype(np.float64)
    assert got.shape == ref["attrs64"].shape == (verts.shape[0], 24)
    bound = T.attr_bound(np.abs(w).max(), ref["n_verts"])[:, None]
    err = np.abs(got - ref["attrs64"])
    # the rows of w sum to 1 within 24 roundings of entries <= 1 (2^-25 each); a mean of such rows does too, then 24 roundings more
    rows = np.abs(got.sum(1) - 1.0)
    row_bound = 24 * 2.0 ** -25 + 24 * bound[:, 0]
    print(f"[simplify attributes] |mean - float64| at most {err.max():.3e} (bound {bound.min():.3e}); |row sum - 1| at most "
          f"{rows.max():.3e} (bound {row_bound.min():.3e})")
    assert (err <= bound).all() and (rows <= row_bound).all()
    again = simplify(v, f, cell=h, attrs=w)[2]["attrs"]
    assert torch.equal(info["attrs"], again)


# ------------------------------------------------------------------------------------------------ 7. a target face count
def test_target_faces_walks_the_references_bisection():
    v, f = S.squashed(4)
    ref = R.simplify_to(v, f, 700)
    got = simplify(v, f, target_faces=700)
    assert got[2]["cell"] == ref["info"]["cell"] and got[2]["passes"] == ref["info"]["passes"] <= 16
    check("squashed(4) to 700 faces", got, ref)
    live = f.shape[0] - got[2]["n_collapsed"]
    print(f"[simplify target 700] {got[2]['passes']} passes, cell {got[2]['cell']:.6f}, {live} faces before, {got[1].shape[0]} after de-duplication")
    assert abs(live - 700) <= 0.02 * 700
    from multiply_amd.simplify import cluster_counts
    assert cluster_counts(*on_device(v, f), got[2]["cell"]) == (got[2]["n_cells"], live)


# ------------------------------------------------------------------------------------------------ 8. ExtractedMesh, the tool
@pytest.fixture(scope="module")
def sphere_mesh():
    from multiply_amd.mesh import ExtractedMesh, marching_cubes
    n = 41
    g = torch.linspace(-1, 1, n, device=DEV)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    vol = 0.7 - torch.sqrt(x * x + 1.3 * y * y + 0.8 * z * z)
    verts, faces = marching_cubes(vol, 0.0)
    return ExtractedMesh(verts, faces, resolution=n - 1)


def test_extracted_mesh_simplify_exports_and_reloads(sphere_mesh, tmp_path):
    from multiply_amd.mesh import ExtractedMesh
    from multiply_amd.metrics import load_ply
    m = sphere_mesh
    assert m.faces.shape[0] > 4000 and m.is_watertight
    s = m.simplify(target_faces=800)
    ref = R.simplify_to(m.vertices, m.faces, 800)
    assert isinstance(s, ExtractedMesh) and s.cell == ref["info"]["cell"] and s.passes == ref["info"]["passes"] <= 16
    check("sphere extraction", (s.vertices_t, s.faces_t, s.info), ref)
    assert s.faces.shape[0] < m.faces.shape[0] and 0 < s.area and len(s.split()) >= 1 and s.is_watertight in (True, False)
    v2, f2 = load_ply(s.export(str(tmp_path / "s.ply")))
    assert np.array_equal(v2, s.vertices) and np.array_equal(f2, s.faces)
    c = m.simplify(cell=4.0)
    assert c.faces.shape[0] < m.faces.shape[0] and c.cell == 4.0
    with pytest.raises(ValueError, match="exactly one"):
        m.simplify()


def test_tool_on_a_file_and_a_folder(sphere_mesh, tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import simplify_mesh as tool
    finally:
        sys.path.pop(0)
    from multiply_amd.metrics import load_ply
    src = tmp_path / "in"
    src.mkdir()
    sphere_mesh.export(str(src / "0000_canonical.ply"))
    sphere_mesh.export(str(src / "0001_canonical.ply"))
    out = tool.main([str(src / "0000_canonical.ply"), str(tmp_path / "one.ply"), "--cell", "3.0"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    v, f = load_ply(str(tmp_path / "one.ply"))
    assert line == out and out["faces_after"] == f.shape[0] < out["faces_before"] == sphere_mesh.faces.shape[0]
    assert out["verts_after"] == v.shape[0] and out["bytes_after"] == os.path.getsize(tmp_path / "one.ply") < out["bytes_before"]
    ref = R.simplify(sphere_mesh.vertices, sphere_mesh.faces, 3.0)
    assert np.array_equal(f, ref["faces"]) and out["cell"] == 3.0
    out = tool.main([str(src), str(tmp_path / "all"), "--faces", "600"])
    assert sorted(out["files"]) == ["0000_canonical.ply", "0001_canonical.ply"] and sorted(os.listdir(tmp_path / "all")) == sorted(out["files"])
    assert out["total"]["faces_after"] == 2 * out["files"]["0000_canonical.ply"]["faces_after"] < out["total"]["faces_before"]
