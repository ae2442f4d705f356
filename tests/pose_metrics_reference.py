"""Float64 restatement of the pose metrics (multiply_amd/pose_metrics.py, csrc/pose_metrics.hip) in numpy, with
numpy.linalg.svd.  The reference project has no such code; these are the published definitions (the module's docstring).
tests/test_pose_metrics_cpu.py pins this file on analytic anchors before anything on the device is compared against it."""
import numpy as np


def umeyama(p, x, constrained=True):
    """(s, R, t) minimising sum |s R p_i + t - x_i|^2 over similarity transforms (Umeyama 1991), p, x (n, 3) float64.
    constrained: det R = +1 (D = diag(1, 1, sign det(V U^T))); False: any orthogonal R (D = I), which also aligns a mirror image."""
    p, x = np.asarray(p, np.float64), np.asarray(x, np.float64)
    mp, mx = p.mean(0), x.mean(0)
    pc, xc = p - mp, x - mx
    H = pc.T @ xc
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    D = np.eye(3)
    if constrained and np.linalg.det(V @ U.T) < 0:
        D[2, 2] = -1.0
    R = V @ D @ U.T
    var = (pc * pc).sum()
    s = (S * np.diag(D)).sum() / var if var > 0 else np.nan
    return s, R, mx - s * R @ mp


def item_errors(p, x, p_root=None, x_root=None, constrained=True):
    """(plain, root-aligned, Procrustes, flag) of one item as mp_pose_errors writes them"""
    p, x = np.asarray(p, np.float64), np.asarray(x, np.float64)
    roots = p_root is not None
    fin = np.isfinite(p).all() and np.isfinite(x).all() and (not roots or (np.isfinite(p_root).all() and np.isfinite(x_root).all()))
    if not fin:
        return np.nan, np.nan, np.nan, 1.0
    plain = np.linalg.norm(p - x, axis=1).mean()
    aligned = np.linalg.norm((p - np.asarray(p_root, np.float64)) - (x - np.asarray(x_root, np.float64)), axis=1).mean() if roots else np.nan
    if (p == p[0]).all():                     # the spread about the mean is 0 exactly: no scale
        return plain, aligned, np.nan, 2.0
    s, R, t = umeyama(p, x, constrained)
    return plain, aligned, np.linalg.norm(s * p @ R.T + t - x, axis=1).mean(), 0.0


def pose_errors(pred, gt, pred_root=None, gt_root=None):
    """(M, 4) float64 of pred, gt (M, n, 3): what mp_pose_errors writes"""
    return np.array([item_errors(pred[m], gt[m], None if pred_root is None else pred_root[m], None if gt_root is None else gt_root[m])
                     for m in range(len(pred))], np.float64).reshape(-1, 4)


def contact_points(verts, faces, c):
    """the two ends (m, 3) of every correspondence on the bodies verts (F, P, V, 3): a's vertex and the point of b's face"""
    v = np.asarray(verts, np.float64)
    a = v[c["frame"], c["person_a"], c["vertex"]]
    tri = v[c["frame"][:, None], c["person_b"][:, None], np.asarray(faces)[c["face"]]]       # (m, 3, 3)
    return a, (np.asarray(c["bary"], np.float64)[:, :, None] * tri).sum(1)


def contact_distance(verts, faces, c):
    """overall mean, per-frame means (NaN for a frame without a correspondence), per-frame counts"""
    F = np.asarray(verts).shape[0]
    a, b = contact_points(verts, faces, c)
    d = np.linalg.norm(a - b, axis=1)
    per, cnt = np.full(F, np.nan), np.zeros(F, np.int64)
    for f in range(F):
        sel = c["frame"] == f
        cnt[f] = sel.sum()
        if cnt[f]:
            per[f] = d[sel].mean()
    return (d.mean() if d.size else np.nan), per, cnt


def depths(root_pos, view=None):
    """z (F, P) of the roots (F, P, 3): the world z, or the third camera coordinate under view (3, 4) / (F, 3, 4)"""
    r = np.asarray(root_pos, np.float64)
    if view is None:
        return r[..., 2]
    w = np.asarray(view, np.float64)
    w = np.broadcast_to(w, (r.shape[0], 3, 4))
    return np.einsum("fk,fpk->fp", w[:, 2, :3], r) + w[:, 2, 3][:, None]


def relations(z, threshold, unit_scale=1.0):
    """rel (F, P (P - 1) / 2) for the pairs p < q in row-major order, and |unit_scale |d| - threshold| per pair"""
    P = z.shape[1]
    i, j = np.triu_indices(P, 1)
    d = z[:, i] - z[:, j]
    return np.where(unit_scale * np.abs(d) < threshold, 0.0, np.sign(d)), np.abs(unit_scale * np.abs(d) - threshold)


def pcdr(z_pred, z_gt, threshold, unit_scale=1.0):
    """(share of equal relations or NaN, per-frame shares, number of pairs)"""
    rp, rg = relations(z_pred, threshold, unit_scale)[0], relations(z_gt, threshold, unit_scale)[0]
    n = rp.size
    per = (rp == rg).mean(1) if rp.shape[1] else np.full(rp.shape[0], np.nan)
    return ((rp == rg).sum() / n if n else np.nan), per, n


def metrics(pred, gt, root=0, unit_scale=1.0, contacts=None, faces=None, view=None, depth_threshold=0.15):
    """the dict of pose_metrics.pose_metrics from GIVEN bodies: pred, gt = dicts of joints (F, P, J, 3) and verts (F, P, V, 3)"""
    F, P = pred["joints"].shape[:2]
    out = {}
    pj, gj = (np.asarray(d["joints"], np.float64).reshape(F * P, -1, 3) for d in (pred, gt))
    pr, gr = pj[:, root], gj[:, root]
    e = pose_errors(pj, gj, pr, gr)
    out.update(mpjpe_global=e[:, 0], mpjpe=e[:, 1], pa_mpjpe=e[:, 2])
    if "verts" in pred and "verts" in gt:
        pv, gv = (np.asarray(d["verts"], np.float64).reshape(F * P, -1, 3) for d in (pred, gt))
        e = pose_errors(pv, gv, pr, gr)
        out.update(mve_global=e[:, 0], mve=e[:, 1], pa_mve=e[:, 2])
    out = {k: (v * unit_scale).reshape(F, P) for k, v in out.items()}
    for k in list(out):
        out["mean_" + k] = np.nanmean(out[k]) if np.isfinite(out[k]).any() else np.nan
    out["pcdr"], out["pcdr_per_frame"], out["n_depth_pairs"] = pcdr(depths(pr.reshape(F, P, 3), view), depths(gr.reshape(F, P, 3), view),
                                                                    depth_threshold, unit_scale)
    if contacts is not None:
        for key, d in (("cd", pred), ("cd_gt", gt)):
            m, per, cnt = contact_distance(d["verts"], faces, contacts)
            out[key], out[key + "_per_frame"] = m * unit_scale, per * unit_scale
        out["n_contacts"], out["n_contacts_per_frame"] = int(cnt.sum()), cnt
    return out
