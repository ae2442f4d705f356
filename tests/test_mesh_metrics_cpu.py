"""The float64 reference of the mesh metrics (tests/mesh_metrics_reference.py) on analytic anchors, and the host code of
multiply_amd/metrics.py that needs no device: the PLY reader, the accepted mesh forms, the header's new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_metrics_reference as R
from tests import mesh_metrics_shapes as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closest_point_in_each_of_the_seven_regions():
    tri = np.array([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    cases = [((-1, -1, 1), (0, 0, 0)),            # vertex a
             ((2, -0.5, 1), (1, 0, 0)),           # vertex b
             ((-0.5, 2, 1), (0, 1, 0)),           # vertex c
             ((0.5, -1, 0), (0.5, 0, 0)),         # edge ab
             ((-1, 0.5, 0), (0, 0.5, 0)),         # edge ac
             ((1, 1, 0), (0.5, 0.5, 0)),          # edge bc
             ((0.25, 0.25, 2), (0.25, 0.25, 0))]  # interior
    for p, q in cases:
        d2, Q = R.closest_points(np.array([p], float), tri)
        assert np.allclose(Q[0, 0], q, atol=1e-15), (p, Q[0, 0])
        assert abs(d2[0, 0] - ((np.array(p) - np.array(q)) ** 2).sum()) < 1e-15
    d2, face, q = R.closest(np.array([[0.25, 0.25, 2.0], [np.nan, 0, 0]]), np.concatenate([tri[:, [0, 0, 0]], tri, tri]))
    assert face.tolist() == [1, -1] and d2[0] == 4.0 and np.isinf(d2[1]) and np.isnan(q[1]).all()      # zero-area never, ties low


def test_reference_distance_agrees_with_the_oracles_independent_formulation():
    from oracle import multiply_oracle as O
    v, f = S.squashed(1)
    pts = np.concatenate([p.numpy() for p in S.point_sets(v, f, 0).values()])
    want = O.mesh_signed_distance(torch.from_numpy(pts), torch.from_numpy(v[f])).abs().numpy()
    got = np.sqrt(R.closest(pts, v[f])[0])
    assert np.abs(got - want).max() < 1e-12 * np.abs(pts).max()


def _square_samples(v, f, n, seed):
    g = np.random.default_rng(seed)
    xy = g.random((n, 2))
    fid = (xy[:, 1] > xy[:, 0]).astype(np.int64)                  # face 0 = (0,1,2): below the diagonal
    return np.concatenate([xy, np.full((n, 1), v[0, 2])], 1), fid


@pytest.mark.parametrize("h", [0.125, 0.3])
def test_parallel_unit_squares(h):
    h, tol = float(np.float32(h)), 1e-13                         # the vertices are fp32; 500 additions in float64
    a, b = S.unit_square(0.0), S.unit_square(h)
    m = R.metrics(a, b, _square_samples(*a, 500, 0), _square_samples(*b, 500, 1), thresholds=(0.5 * h, 2.0 * h))
    for k in ("accuracy", "completeness", "p2s", "chamfer", "hausdorff"):
        assert abs(m[k] - h) < tol, k
    assert abs(m["chamfer_sq"] - 2 * h * h) < tol
    assert m["normal_consistency"] == 1.0 and m["normal_consistency_signed"] == 1.0
    assert m["precision"] == [0.0, 1.0] and m["recall"] == [0.0, 1.0] and m["f_score"] == [0.0, 1.0]
    s = R.metrics(a, b, _square_samples(*a, 500, 0), _square_samples(*b, 500, 1), thresholds=(3.0 * h,), unit_scale=2.0)
    assert abs(s["chamfer"] - 2 * h) < tol and abs(s["chamfer_sq"] - 8 * h * h) < tol and s["precision"] == [1.0]


def test_mesh_against_itself():
    v, f = S.squashed(1)
    g = np.random.default_rng(0)
    fid = g.integers(0, f.shape[0], 300)
    w = g.dirichlet([1, 1, 1], 300)
    pts = (v[f][fid].astype(np.float64) * w[:, :, None]).sum(1)
    m = R.metrics((v, f), (v, f), (pts, fid), (pts, fid), thresholds=(1e-9,))
    assert m["chamfer"] < 1e-15 and m["hausdorff"] < 1e-15 and m["chamfer_sq"] < 1e-30
    # an interior point's closest face is its own: the normals agree; (points on edges may answer with the neighbour)
    assert m["normal_consistency"] > 0.99 and m["f_score"] == [1.0]


def test_volume_iou_of_offset_boxes_is_the_hand_count():
    """[0,1]^3 and the same box shifted by (0.5, 0.3, 0), 6 cells per axis over [0,1.5] x [0,1.3] x [0,1], centres
    x = .125, .375, .., 1.375; y = .1083, .325, .5417, .7583, .975, 1.1917; z = 1/12, 3/12, .., 11/12.  Inside A: the 4 x below 1,
    the 5 y below 1, all 6 z: 120; B: the 4 x above .5, the 5 y above .3: 120; both: x in {.625,.875}, the 4 y in (.3,1): 48.
    Union 192: IoU 1/4.  No centre lies on a face, and the shift in y keeps the (y,z) of the centres off the diagonals of the
    boxes' x faces, where the device's ray-parity sign has no right answer."""
    a, b = S.box([0, 0, 0], [1, 1, 1]), S.box([0.5, 0.3, 0], [1.5, 1.3, 1])
    from multiply_amd.smpl_init import mesh_is_closed
    assert mesh_is_closed(a[1]) and abs(R.solid_angle_winding(np.array([[0.5, 0.5, 0.5]]), a[0][a[1]])[0] - 1.0) < 1e-12
    P = R.lattice([0, 0, 0], [1.5, 1.3, 1], 6)
    ia, ib = R.inside(P, a[0][a[1]]), R.inside(P, b[0][b[1]])
    assert (int(ia.sum()), int(ib.sum()), int((ia & ib).sum())) == (120, 120, 48)
    assert R.volume_iou(a, b, 6) == 0.25
    assert R.volume_iou(a, a, 5) == 1.0
    assert R.volume_iou(a, S.box([2, 0.3, 0], [3, 1.3, 1]), 9) == 0.0


def test_load_ply_round_trips_export_and_reads_ascii(tmp_path):
    from multiply_amd import metrics
    from multiply_amd.mesh import ExtractedMesh
    v, f = S.squashed(1)
    path = ExtractedMesh(torch.from_numpy(v), torch.from_numpy(f)).export(str(tmp_path / "m.ply"))
    gv, gf = metrics.load_ply(path)
    assert gv.dtype == np.float32 and gf.dtype == np.int64 and np.array_equal(gv, v) and np.array_equal(gf, f)
    asc = tmp_path / "a.ply"
    asc.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\n"
                   "property float z\nproperty uchar red\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
                   "0 0 0 255\n1 0 0.5 0\n1 1 0 7\n0 1 -2.25 9\n3 0 1 2\n3 0 2 3\n")
    av, af = metrics.load_ply(asc)
    assert np.array_equal(av, np.array([[0, 0, 0], [1, 0, 0.5], [1, 1, 0], [0, 1, -2.25]], np.float32))
    assert np.array_equal(af, np.array([[0, 1, 2], [0, 2, 3]]))
    (tmp_path / "quad.ply").write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                                       "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                                       "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError):
        metrics.load_ply(tmp_path / "quad.ply")
    # the three accepted forms give the same mesh
    for form in (path, (v, f), (torch.from_numpy(v), torch.from_numpy(f)), ExtractedMesh(torch.from_numpy(v), torch.from_numpy(f))):
        mv, mf = metrics.as_mesh(form, device="cpu")
        assert mv.dtype == torch.float32 and mf.dtype == torch.int64 and np.array_equal(mv.numpy(), v) and np.array_equal(mf.numpy(), f)


def test_header_declares_the_new_entry_points_and_metrics_imports_without_a_device():
    import ctypes
    from multiply_amd import hip, metrics
    protos = hip.header_prototypes()
    want = {"mp_mesh_closest": 8, "mp_mesh_index_closest": 10, "mp_mesh_index_point_keys": 5, "mp_mesh_metric_reduce": 10}
    for name, nargs in want.items():
        assert name in protos and protos[name][0] is ctypes.c_int and len(protos[name][1]) == nargs, name
    assert protos["mp_mesh_index_closest"][1][:5] == [hip.DevPtr, ctypes.c_int, hip.DevPtr, ctypes.c_int, hip.DevPtr]
    for fn in ("load_ply", "surface_samples", "directed", "mesh_metrics", "volume_iou"):
        assert callable(getattr(metrics, fn))
    assert "closest" in dir(hip.MeshIndex) and callable(hip.mesh_closest)
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    assert re.search(r"int mp_mesh_closest\(const float\* pts, int n, const float\* face_verts, int n_faces, float\* d2, int\* face", hdr)


def test_eval_tool_parses_its_arguments(monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_meshes", os.path.join(REPO, "tools", "eval_meshes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from multiply_amd import hip, metrics
    seen = {}
    monkeypatch.setattr(hip, "require_device", lambda: None)
    monkeypatch.setattr(metrics, "mesh_metrics", lambda *a, **k: seen.update(a=a, k=k) or {"chamfer": 0.0})
    assert mod.main(["p.ply", "g.ply", "--samples", "10", "--thresholds", "0.01", "0.02", "--iou-res", "32", "--scale", "100"]) == {"chamfer": 0.0}
    assert seen["a"] == ("p.ply", "g.ply") and seen["k"] == dict(n_samples=10, thresholds=[0.01, 0.02], seed=0, unit_scale=100.0,
                                                                  iou_resolution=32)
