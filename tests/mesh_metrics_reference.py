"""Float64 reference of the closest-face query and the mesh metrics (multiply_amd/metrics.py, csrc/mesh_closest.hip).  The
reference project has no such code; this restates the published definitions in numpy.  tests/test_mesh_metrics_cpu.py pins it on
analytic anchors before anything on the device is compared against it.

closest_points is Ericson's region classification (Real-Time Collision Detection 5.1.5) in float64, vectorised: in float64 the
classification's rounding is ~1e-16 M, nine orders below the fp32 slack it is compared at.  oracle.multiply_oracle's distance
(plane projection + three segments) is an independent formulation; the CPU test checks the two against each other."""
import numpy as np


def closest_points(P, FV):
    """P (n,3), FV (F,3,3) -> d2 (n,F), Q (n,F,3) float64: the closest point of every face to every point.  A face of zero area
    (cross product exactly 0) gets NaN."""
    P, FV = np.asarray(P, np.float64), np.asarray(FV, np.float64)
    return _closest(P[:, None, :], FV[None, :, 0], FV[None, :, 1], FV[None, :, 2])


def closest_points_paired(P, FV):
    """P (n,3), FV (n,3,3) -> d2 (n,), Q (n,3): point i against face i alone"""
    P, FV = np.asarray(P, np.float64), np.asarray(FV, np.float64)
    return _closest(P, FV[:, 0], FV[:, 1], FV[:, 2])


def _closest(p, a, b, c):
    with np.errstate(all="ignore"):                              # non-finite points and zero-area faces answer NaN, quietly
        return _closest_quiet(p, a, b, c)


def _closest_quiet(p, a, b, c):
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        t_ab, t_ac = d1 / (d1 - d3), d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        Q = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    full = lambda x: np.broadcast_to(x, ap.shape)
    cands = [full(a), full(b), a + t_ab[..., None] * ab, full(c), a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b)]
    taken = np.zeros(d1.shape, bool)
    for cond, cand in zip(conds, cands):
        use = cond & ~taken
        Q = np.where(use[..., None], cand, Q)
        taken |= cond
    flat = (np.cross(ab, ac) == 0).all(-1)
    Q = np.where(flat[..., None], np.nan, Q)
    return dot(p - Q, p - Q), Q


def closest(P, FV, chunk=512):
    """per point: d2 (n,), face (n,) = the lowest id among the faces attaining the minimum (-1: none), q (n,3); float64"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    n = P.shape[0]
    d2, face, q = np.full(n, np.inf), np.full(n, -1, np.int64), np.full((n, 3), np.nan)
    for s in range(0, n, chunk):
        D, Q = closest_points(P[s:s + chunk], FV)
        D = np.where(np.isnan(D), np.inf, D)
        k = D.argmin(1)                                          # the first minimum = the lowest id
        m = np.isfinite(D[np.arange(k.shape[0]), k])
        d2[s:s + chunk] = np.where(m, D[np.arange(k.shape[0]), k], np.inf)
        face[s:s + chunk] = np.where(m, k, -1)
        q[s:s + chunk] = np.where(m[:, None], Q[np.arange(k.shape[0]), k], np.nan)
    return d2, face, q


def all_d2(P, FV, chunk=512):
    """d2 (n,F) float64 of every point to every face (NaN: zero-area face)"""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    return np.concatenate([closest_points(P[s:s + chunk], FV)[0] for s in range(0, P.shape[0], chunk)]) if P.shape[0] else \
        np.zeros((0, np.asarray(FV).shape[0]))


def face_normals(FV):
    """unit normals (F,3) float64, (b - a) x (c - a); 0 for a zero-area face"""
    FV = np.asarray(FV, np.float64)
    n = np.cross(FV[:, 1] - FV[:, 0], FV[:, 2] - FV[:, 0])
    l = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(l > 0, n / np.where(l > 0, l, 1.0), 0.0)


def reduce(d2, face, normals, fnormals, thresholds=()):
    """what mp_mesh_metric_reduce returns, float64: mean d, mean d2, max d, mean n.n', mean |n.n'|, counted, left out, counts"""
    d2, face = np.asarray(d2, np.float64), np.asarray(face)
    ok = face >= 0
    d = np.sqrt(d2[ok])
    nn = (np.asarray(normals, np.float64)[ok] * np.asarray(fnormals, np.float64)[face[ok]]).sum(1)
    k = int(ok.sum())
    mean = lambda x: float(x.sum() / k) if k else 0.0
    return [mean(d), mean(d2[ok]), float(d.max()) if k else 0.0, mean(nn), mean(np.abs(nn)), float(k), float((~ok).sum())] + \
           [float((d < t).sum()) for t in thresholds]


def solid_angle_winding(P, FV):
    """generalised winding number (n,) of the closed, outward-oriented mesh around every point (Van Oosterom & Strackee 1983)"""
    P, FV = np.asarray(P, np.float64), np.asarray(FV, np.float64)
    a, b, c = (FV[None, :, i] - P[:, None, :] for i in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)


def inside(P, FV, chunk=2048):
    """strictly inside the closed mesh: winding number above 1/2 and not on the surface -- nearer than 1e-12 M, M the largest
    |coordinate|: the float64 rounding of the closest point (a point in a face's plane gets ~1e-16, not 0), five orders below
    what fp32 coordinates can tell apart"""
    P = np.asarray(P, np.float64)
    out = np.zeros(P.shape[0], bool)
    on = (1e-12 * max(np.abs(P).max(), np.abs(np.asarray(FV)).max())) ** 2
    for s in range(0, P.shape[0], chunk):
        p = P[s:s + chunk]
        out[s:s + chunk] = (solid_angle_winding(p, FV) > 0.5) & (closest(p, FV)[0] > on)
    return out


def lattice(lo, hi, R):
    """the R^3 points of metrics.volume_iou: the cell centres of [lo, hi] split R times per axis; float32 as the device sees them"""
    ax = [(np.float64(np.float32(lo[k])) + (np.arange(R) + 0.5) * ((np.float64(np.float32(hi[k])) - np.float64(np.float32(lo[k]))) / R))
          .astype(np.float32) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def volume_iou(pred, gt, R):
    (pv, pf), (gv, gf) = pred, gt
    lo, hi = np.minimum(pv.min(0), gv.min(0)), np.maximum(pv.max(0), gv.max(0))
    P = lattice(lo, hi, R)
    a, b = inside(P, pv[pf]), inside(P, gv[gf])
    union = int((a | b).sum())
    return float((a & b).sum() / union) if union else 0.0


def metrics(pred, gt, samples_pred, samples_gt, thresholds=(), unit_scale=1.0, iou_resolution=None, reported=None):
    """the dict of metrics.mesh_metrics from GIVEN samples: samples_x = (points (n,3), faces (n,)) ON mesh x (the normal of a
    sample is its face's).  The distances are the float64 minima over all faces; the normal n' is that of the float64 closest
    face, or of the faces in reported = (faces for pred's samples, faces for gt's samples) -- where two faces are equally near
    (an edge, a vertex) either is a closest face, and the query under test says which one it took."""
    (pv, pf), (gv, gf) = [(np.asarray(v, np.float64), np.asarray(f)) for v, f in (pred, gt)]
    s, out, part = float(unit_scale), {}, {}
    for k, (name, (pts, fid), (sv, sf), (tv, tf)) in enumerate((("accuracy", samples_pred, (pv, pf), (gv, gf)),
                                                                ("completeness", samples_gt, (gv, gf), (pv, pf)))):
        d2, face, _ = closest(pts, tv[tf])
        face = face if reported is None else np.where(face >= 0, np.asarray(reported[k]), -1)
        part[name] = reduce(d2, face, face_normals(sv[sf])[np.asarray(fid)], face_normals(tv[tf]), [t / s for t in thresholds])
    a, c = part["accuracy"], part["completeness"]
    out.update(accuracy=s * a[0], completeness=s * c[0], p2s=s * c[0], chamfer=s * 0.5 * (a[0] + c[0]),
               chamfer_sq=s * s * (a[1] + c[1]), hausdorff=s * max(a[2], c[2]), normal_consistency=0.5 * (a[4] + c[4]),
               normal_consistency_signed=0.5 * (a[3] + c[3]))
    P = [a[7 + k] / a[5] if a[5] else 0.0 for k in range(len(thresholds))]
    Rc = [c[7 + k] / c[5] if c[5] else 0.0 for k in range(len(thresholds))]
    out.update(thresholds=[float(t) for t in thresholds], precision=P, recall=Rc,
               f_score=[2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, Rc)])
    if iou_resolution:
        out["volume_iou"] = volume_iou((pv.astype(np.float32), pf), (gv.astype(np.float32), gf), int(iou_resolution))
    return out
