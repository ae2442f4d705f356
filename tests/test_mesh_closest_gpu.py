"""Closest face and closest point (csrc/mesh_closest.hip brute force, csrc/mesh_index.hip through the face index): the two return
the same bits -- with and without the Hilbert ordering of the query points, through the C entry points and through
hip.MeshIndex.closest --, agree with the float64 reference (tests/mesh_metrics_reference.py) within the kernel's own slack
(tests/tolerances_mesh_metrics.py), break ties towards the lower face id, never report a zero-area face, and answer non-finite
points with (-1, +inf, NaN)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import mesh_metrics_reference as R
from tests import mesh_metrics_shapes as S
from tests import tolerances_mesh_metrics as TOL

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
ODD = [[NAN, 0.1, 0.2], [0.1, NAN, NAN], [INF, 0.0, 0.1], [-INF, 0.0, 0.1], [0.1, INF, 0.0], [0.0, 0.1, -INF], [INF, -INF, INF]]


def _meshes():
    """{name: (face_verts (F,3,3) float32 numpy, zero-area face ids)}"""
    ico_v, ico_f = S.icosphere(0, base=20)
    ico = ico_v[ico_f]
    out = {"triangle": (np.array([[[0.1, 0.0, 0.0], [1.0, 0.2, 0.0], [0.3, 1.0, 0.5]]], np.float32), []),
           "cube": (S.cube()[0][S.cube()[1]], []),
           "icosahedron": (ico, []),
           "squashed(2)": ((lambda v, f: v[f])(*S.squashed(2)), []),
           "planar grid": ((lambda v, f: v[f])(*S.quad_grid(2)), []),
           "doubled icosahedron": (np.concatenate([ico, ico]), [])}
    # zero-area faces in FRONT of the faces they touch (a tie would go to them) and in the middle: a point, and an edge run twice
    z = np.concatenate([ico[5:6][:, [0, 0, 0]], ico[:10], ico[7:8][:, [0, 1, 1]], ico[10:]])
    out["with zero-area faces"] = (z, [0, 11])
    return out


def _points(fv, seed):
    """the point sets of the index tests around the mesh, then the non-finite points; [(name, start, stop)]"""
    v = fv.reshape(-1, 3)
    f = np.arange(v.shape[0]).reshape(-1, 3)
    keep = np.array([i for i in range(f.shape[0]) if np.any(np.cross(fv[i, 1] - fv[i, 0], fv[i, 2] - fv[i, 0]) != 0)])
    sets = S.point_sets(v, f[keep], seed)
    names, parts, at = [], [], 0
    for k, p in sets.items():
        names.append((k, at, at + p.shape[0]))
        parts.append(p)
        at += p.shape[0]
    names.append(("non-finite", at, at + len(ODD)))
    parts.append(torch.tensor(ODD))
    return torch.cat(parts).contiguous(), names


def brute(pts, fv, face=True, q=True):
    from multiply_amd import hip
    n = pts.shape[0]
    d2 = torch.full((n,), -7.0, device="cuda")
    fa = torch.full((n,), -7, dtype=torch.int32, device="cuda") if face else None
    qq = torch.full((n, 3), -7.0, device="cuda") if q else None
    hip.lib().mp_mesh_closest(pts, n, fv, fv.shape[0], d2, fa, qq, hip.stream())
    return d2, fa, qq


def build(fv):
    """the C entry points one by one, as hip.MeshIndex drives them: (index buffer, order)"""
    from multiply_amd import hip
    L, F = hip.lib(), fv.shape[0]
    buf = torch.empty(int(L.mp_mesh_index_bytes(F)), dtype=torch.uint8, device="cuda")
    keys = torch.empty(F, dtype=torch.int32, device="cuda")
    L.mp_mesh_index_keys(fv, F, buf, keys, hip.stream())
    order = torch.sort(keys, stable=True).indices
    L.mp_mesh_index_build(fv, F, order, buf, hip.stream())
    return buf, order


def indexed(pts, fv, built=None, use_order=True, sort_points=False):
    from multiply_amd import hip
    L, F, n = hip.lib(), fv.shape[0], pts.shape[0]
    buf, order = build(fv) if built is None else built
    perm = None
    if sort_points:
        keys = torch.empty(n, dtype=torch.int32, device="cuda")
        L.mp_mesh_index_point_keys(pts, n, buf, keys, hip.stream())
        perm = torch.sort(keys).indices
        pts = pts[perm].contiguous()
    d2 = torch.full((n,), -7.0, device="cuda")
    fa = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    qq = torch.full((n, 3), -7.0, device="cuda")
    L.mp_mesh_index_closest(pts, n, buf, F, order if use_order else None, d2, fa, qq, None, hip.stream())
    if perm is not None:
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(n, device="cuda")
        d2, fa, qq = d2[inv], fa[inv], qq[inv]
    return d2, fa, qq


def same_bits(a, b):
    """equal bits, NaNs and the signs of zeros included"""
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def cases():
    """per mesh: the points, brute force's answer and the float64 reference, computed once and left unchanged"""
    out = {}
    for k, (name, (fv, zero)) in enumerate(_meshes().items()):
        pts, names = _points(fv, k)
        fvd, pd = torch.from_numpy(fv).reshape(-1, 9).cuda().contiguous(), pts.cuda().contiguous()
        got = brute(pd, fvd)
        torch.cuda.synchronize()
        out[name] = dict(fv=fv, zero=zero, pts=pts, sets=names, fvd=fvd, pd=pd, brute=got, D2=R.all_d2(pts.numpy(), fv))
    return out


MESHES = list(_meshes())


@pytest.mark.parametrize("name", MESHES)
def test_index_equals_brute_force(name, cases):
    from multiply_amd import hip
    c = cases[name]
    built = build(c["fvd"])
    for sort_points in (False, True):
        got = indexed(c["pd"], c["fvd"], built, sort_points=sort_points)
        bad = (got[0].view(torch.int32) != c["brute"][0].view(torch.int32)) | (got[1] != c["brute"][1])
        print(f"[closest] {name}: {c['pd'].shape[0]} points x {c['fv'].shape[0]} faces, sorted points {sort_points}: {int(bad.sum())} differ"
              + (f"; first {c['pts'][bad.cpu()][0].tolist()}" if bad.any() else ""))
        assert same_bits(got, c["brute"]), (name, sort_points)
    index = hip.MeshIndex(torch.from_numpy(c["fv"]).cuda())
    assert torch.equal(index.order, built[1])
    for sort_points in (False, True, None):
        assert same_bits(index.closest(c["pd"], sort_points=sort_points), c["brute"]), (name, sort_points)
    assert same_bits(hip.mesh_closest(c["pd"], torch.from_numpy(c["fv"]).cuda(), index=index), c["brute"])
    assert same_bits(hip.mesh_closest(c["pd"], torch.from_numpy(c["fv"]).cuda()), c["brute"])
    d2, fa, qq = index.closest(c["pd"], want_face=False, want_point=False)
    assert fa is None and qq is None and same_bits([d2], c["brute"][:1])
    assert same_bits([brute(c["pd"], c["fvd"], face=False, q=False)[0]], c["brute"][:1])


def test_index_equals_brute_force_on_a_deep_tree():
    """8 192 faces: 1 024 leaves, the inner levels built by more than one launch"""
    v, f = S.squashed(5, base=8)
    assert f.shape[0] == 8192
    fvd = torch.from_numpy(v[f]).reshape(-1, 9).cuda().contiguous()
    pts = torch.cat(list(S.point_sets(v, f, 5).values()) + [torch.tensor(ODD)]).cuda().contiguous()
    want, built = brute(pts, fvd), build(fvd)
    visits = torch.zeros(pts.shape[0], 2, dtype=torch.int32, device="cuda")
    from multiply_amd import hip
    index = hip.MeshIndex(fvd)
    for sort_points in (False, True):
        assert same_bits(indexed(pts, fvd, built, sort_points=sort_points), want)
        assert same_bits(index.closest(pts, visits=visits, sort_points=sort_points), want)
        vm = visits[:-len(ODD)].float().mean(0).tolist()
        print(f"[closest] 8192 faces: boxes/pt {vm[0]:.1f} faces/pt {vm[1]:.1f} (sorted points {sort_points})")
        assert 8 <= vm[1] < 8192 / 4 and int(visits[-len(ODD):].sum()) == 0          # sub-linear; non-finite points do not walk
        first = visits.clone() if not sort_points else first
    assert torch.equal(first, visits)                                               # visits come back in the caller's order


@pytest.mark.parametrize("name", MESHES)
def test_against_float64(name, cases):
    """every finite point of every set: the distance, the reported face (set membership: ties between the faces of an edge or a
    vertex are by construction), the closest point on that face"""
    c = cases[name]
    d2, fa, qq = (t.cpu().numpy() for t in c["brute"])
    for sname, s0, s1 in c["sets"]:
        if sname == "non-finite":
            continue
        P, D2 = c["pts"][s0:s1].numpy().astype(np.float64), c["D2"][s0:s1]
        M = TOL.coordinate_scale(P, c["fv"])
        delta = TOL.delta(M)
        d64 = np.sqrt(np.nanmin(D2, axis=1))
        f = fa[s0:s1].astype(np.int64)
        assert (f >= 0).all() and (f < c["fv"].shape[0]).all()
        e_d = np.abs(np.sqrt(d2[s0:s1].astype(np.float64)) - d64).max()
        e_f = (np.sqrt(D2[np.arange(P.shape[0]), f]) - d64).max()
        q = qq[s0:s1].astype(np.float64)
        e_q = np.sqrt(R.closest_points_paired(q, c["fv"][f])[0]).max()
        e_pq = np.abs(np.linalg.norm(P - q, axis=1) - np.sqrt(d2[s0:s1].astype(np.float64))).max()
        print(f"[closest vs float64] {name} / {sname}: M {M:.2f} delta {delta:.2e} | distance {e_d:.2e}  face {e_f:.2e} (<= 2 delta)  "
              f"q off its face {e_q:.2e}  | |p-q| - d | {e_pq:.2e}")
        assert e_d <= delta and e_f <= TOL.face_membership(M) and e_q <= delta and e_pq <= delta, (name, sname)


def test_ties_go_to_the_lower_face_id_and_order_null_reports_sorted_slots(cases):
    c = cases["doubled icosahedron"]
    fa = c["brute"][1].cpu()
    finite = torch.isfinite(c["pts"]).all(1)
    assert int(fa[finite].max()) < 20 and int(fa[finite].min()) >= 0
    # the faces of a vertex tie: the lowest of them is reported (float64 names the tied set; fp32 picks inside it)
    s0, s1 = next((a, b) for k, a, b in c["sets"] if k == "on vertices")
    tied = c["D2"][s0:s1] == 0.0
    assert tied.sum(1).min() >= 10 and np.array_equal(fa[s0:s1].numpy(), tied.argmax(1))
    built = build(c["fvd"])
    slots = indexed(c["pd"], c["fvd"], built, use_order=False)
    ok = finite.cuda()
    assert torch.equal(slots[0].view(torch.int32), c["brute"][0].view(torch.int32))
    assert bool((slots[1][~ok] == -1).all())
    # a slot's face is order[slot].  Ties are broken on the slot numbers now, so it is A closest face (float64, within the
    # kernel's slack), and where only a face and its twin f + 20 are that near, the reported face or its twin
    mine = built[1][slots[1][ok].long()].cpu().numpy()
    D2 = c["D2"][finite.numpy()]
    d64 = np.sqrt(D2.min(1))
    slack = TOL.face_membership(TOL.coordinate_scale(c["pts"][finite].numpy(), c["fv"]))
    assert (np.sqrt(D2[np.arange(mine.shape[0]), mine]) <= d64 + slack).all()
    alone = (np.sqrt(D2) <= (d64 + slack)[:, None]).sum(1) == 2
    assert alone.mean() > 0.25 and np.array_equal(mine[alone] % 20, fa[finite].numpy()[alone])


def test_zero_area_faces_are_never_reported(cases):
    from multiply_amd import hip
    c = cases["with zero-area faces"]
    fa = c["brute"][1].cpu()
    finite = torch.isfinite(c["pts"]).all(1)
    assert not np.isin(fa[finite].numpy(), c["zero"]).any() and int(fa[finite].min()) >= 0
    # nothing but zero-area faces: no answer for anybody
    flat = torch.from_numpy(c["fv"][c["zero"]]).reshape(-1, 9).cuda().contiguous()
    for got in (brute(c["pd"], flat), indexed(c["pd"], flat), hip.MeshIndex(flat).closest(c["pd"], sort_points=True)):
        assert bool((got[1] == -1).all()) and bool(torch.isposinf(got[0]).all()) and bool(torch.isnan(got[2]).all())


@pytest.mark.parametrize("name", ["squashed(2)", "triangle"])
def test_non_finite_points_have_no_answer_and_disturb_nobody(name, cases):
    c = cases[name]
    s0, s1 = next((a, b) for k, a, b in c["sets"] if k == "non-finite")
    d2, fa, qq = c["brute"]
    assert bool((fa[s0:s1] == -1).all()) and bool(torch.isposinf(d2[s0:s1]).all()) and bool(torch.isnan(qq[s0:s1]).all())
    mixed = c["pd"].clone()
    at = torch.tensor([3, 64, 70, 131, 200, 333, 400], device="cuda")
    mixed[at] = torch.tensor(ODD, device="cuda")
    keep = torch.ones(mixed.shape[0], dtype=torch.bool, device="cuda")
    keep[at] = False
    for got in (brute(mixed, c["fvd"]), indexed(mixed, c["fvd"], sort_points=True)):
        assert same_bits([t[keep] for t in got], [t[keep] for t in c["brute"]])
        assert bool((got[1][at] == -1).all()) and bool(torch.isposinf(got[0][at]).all()) and bool(torch.isnan(got[2][at]).all())


@pytest.mark.parametrize("n", [0, 1, 65])
def test_small_point_counts(n, cases):
    from multiply_amd import hip
    c = cases["icosahedron"]
    pts = c["pd"][:n].contiguous()
    want = [t[:n] for t in c["brute"]]
    index = hip.MeshIndex(c["fvd"])
    for got in (brute(pts, c["fvd"]), indexed(pts, c["fvd"]), indexed(pts, c["fvd"], sort_points=True), index.closest(pts, sort_points=True),
                index.closest(pts, sort_points=False), hip.mesh_closest(pts, c["fvd"])):
        assert got[0].shape == (n,) and got[1].shape == (n,) and got[2].shape == (n, 3) and same_bits(got, want)


def test_two_calls_give_identical_bits(cases):
    c = cases["squashed(2)"]
    assert same_bits(brute(c["pd"], c["fvd"]), c["brute"])
    built = build(c["fvd"])
    assert same_bits(indexed(c["pd"], c["fvd"], built), indexed(c["pd"], c["fvd"], built))


def test_status_codes(cases):
    """-1 without a launch for a NULL required argument, n < 0, n_faces <= 0; 0 without a launch for n == 0 (outputs untouched)"""
    from multiply_amd import hip
    hip.require_device()
    raw = ctypes.CDLL(hip.LIB_PATH)                              # no errcheck: the status itself
    for name, (rt, at) in hip.header_prototypes().items():
        if name in ("mp_mesh_closest", "mp_mesh_index_closest", "mp_mesh_index_point_keys", "mp_mesh_metric_reduce"):
            getattr(raw, name).restype, getattr(raw, name).argtypes = rt, at
    c = cases["icosahedron"]
    pts, fv, F, n, st = c["pd"], c["fvd"], 20, c["pd"].shape[0], hip.stream()
    buf, order = build(fv)
    d2 = torch.full((n,), -7.0, device="cuda")
    fa = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    q = torch.full((n, 3), -7.0, device="cuda")
    keys = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    assert raw.mp_mesh_closest(None, n, fv, F, d2, fa, q, st) == -1 and raw.mp_mesh_closest(pts, n, None, F, d2, fa, q, st) == -1
    assert raw.mp_mesh_closest(pts, n, fv, F, None, fa, q, st) == -1 and raw.mp_mesh_closest(pts, -1, fv, F, d2, fa, q, st) == -1
    assert raw.mp_mesh_closest(pts, n, fv, 0, d2, fa, q, st) == -1 and raw.mp_mesh_closest(pts, 0, fv, F, d2, fa, q, st) == 0
    assert raw.mp_mesh_index_closest(None, n, buf, F, order, d2, fa, q, None, st) == -1
    assert raw.mp_mesh_index_closest(pts, n, None, F, order, d2, fa, q, None, st) == -1
    assert raw.mp_mesh_index_closest(pts, n, buf, F, order, None, fa, q, None, st) == -1
    assert raw.mp_mesh_index_closest(pts, -1, buf, F, order, d2, fa, q, None, st) == -1
    assert raw.mp_mesh_index_closest(pts, n, buf, 0, order, d2, fa, q, None, st) == -1
    assert raw.mp_mesh_index_closest(pts, 0, buf, F, order, d2, fa, q, None, st) == 0
    assert raw.mp_mesh_index_point_keys(pts, -1, buf, keys, st) == -1 and raw.mp_mesh_index_point_keys(pts, n, None, keys, st) == -1
    assert raw.mp_mesh_index_point_keys(pts, n, buf, None, st) == -1 and raw.mp_mesh_index_point_keys(pts, 0, buf, keys, st) == 0
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    fn = torch.zeros(F, 3, device="cuda")
    assert raw.mp_mesh_metric_reduce(d2, fa, q, fn, n, F, None, 1, out, st) == -1           # a threshold count without thresholds
    assert raw.mp_mesh_metric_reduce(d2, fa, q, fn, n, F, None, 9, out, st) == -1
    assert raw.mp_mesh_metric_reduce(d2, fa, q, fn, n, F, None, 0, None, st) == -1
    assert raw.mp_mesh_metric_reduce(None, fa, q, fn, n, F, None, 0, out, st) == -1
    assert raw.mp_mesh_metric_reduce(d2, fa, q, fn, -1, F, None, 0, out, st) == -1
    torch.cuda.synchronize()
    assert bool((d2 == -7).all()) and bool((fa == -7).all()) and bool((q == -7).all()) and bool((keys == -7).all())
    assert bool((out == 0).all())
    with pytest.raises(RuntimeError, match="code -1"):                                        # the binding raises on it
        hip.lib().mp_mesh_closest(pts, -1, fv, F, d2, fa, q, st)
