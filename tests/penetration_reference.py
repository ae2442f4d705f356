"""The mesh-free interpenetration term (multiply_amd/train.py Interpenetration, csrc/penetration.hip) restated on the oracle's
pieces: servers[p].forward, O.query_weights, O.skinning and the persons' implicit networks, the way _surface_loss of
tests/test_smpl_surface_pose_grad_gpu.py restates its term.

    X_p  = smpl_verts_p[pen_idx_p]                     attached to p's body model
    (nn, outlier) = O.query_weights(X_p, pv_q)         pv_q, the skinning weights and cond_q detached
    x_c  = O.skinning(x, w_nn, tfs_q, inverse=True)    tfs_q attached to q's body model
    s    = sdf_q(x_c; cond_q)
    L_pq = sum over {not outlier, s < 0} of s^2        L = sum over the ordered pairs p != q

The body models run in the oracle's float32 (or, `servers=`, in float64 copies of them); everything behind the posed vertices
and transforms runs in `dtype` (float64 for the comparisons)."""
import contextlib
import copy

import numpy as np
import torch

from oracle import multiply_oracle as O

OUTLIER = 0.1               # deformer.py:41-49
NEAR_THRESHOLD = 1e-5       # exclusion: |nearest-vertex distance - 0.1| within this
NEAR_TIE = 1e-6             # exclusion: the two nearest vertices within this of each other
EXCLUDED_MAX_FRACTION, EXCLUDED_MAX = 0.005, 8


def two_nearest(x, verts, chunk=512):
    """distances (n,2) to the two nearest vertices and the id (n,) of the nearest (ties: lowest id), in x's dtype"""
    d, i = [], []
    for s in range(0, x.shape[0], chunk):
        d2 = ((x[s:s + chunk, None, :] - verts[None, :, :]) ** 2).sum(-1)
        v, k = torch.topk(d2, 2, dim=1, largest=False)
        d.append(v.sqrt())
        i.append(d2.argmin(1))
    if not d:
        return x.new_zeros(0, 2), torch.zeros(0, dtype=torch.long)
    return torch.cat(d), torch.cat(i)


def probe(x, pv_q, tfs_q, skin_w):
    """the geometry front end of one pair: x (n,3) probe points (may carry a graph), q's posed vertices (detached by the caller),
    transforms (24,4,4) and skinning weights -> dict(probed (n,) bool, nn (n,) long (-1: outlier), xc (m,3) of the m probed points
    in ascending order, ids (m,), excluded (n,) bool: the points a float32 implementation may decide differently)"""
    n = x.shape[0]
    xd = x.detach()
    probed = torch.zeros(n, dtype=torch.bool)
    nn = torch.full((n,), -1, dtype=torch.long)
    excluded = torch.zeros(n, dtype=torch.bool)
    # a point outside the box of q's vertices grown by more than the outlier radius has no vertex within it: an outlier, exactly
    lo, hi = pv_q.min(0).values - 0.11, pv_q.max(0).values + 0.11
    cand = ((xd >= lo) & (xd <= hi)).all(1).nonzero().flatten()
    ids = cand[:0]
    xc = x[:0]
    if cand.numel():
        w, outlier, idx = O.query_weights(xd[cand], pv_q, skin_w)
        d12, first = two_nearest(xd[cand], pv_q)
        assert torch.equal(first, idx), "O.query_weights' nearest vertex is the argmin"
        near = (d12[:, 0] - OUTLIER).abs() <= NEAR_THRESHOLD
        tie = ~outlier & ((d12[:, 1] - d12[:, 0]) <= NEAR_TIE)
        excluded[cand] = near | tie
        ids = cand[~outlier]
        probed[ids] = True
        nn[ids] = idx[~outlier]
        xc = O.skinning(x[ids], w[~outlier].to(x.dtype), tfs_q, inverse=True)
    return dict(probed=probed, nn=nn, xc=xc, ids=ids, excluded=excluded)


def servers64(oracle):
    """float64 copies of the oracle's body models (use under float64_default())"""
    out = []
    for srv in oracle.servers:
        s = copy.copy(srv)
        s.T = copy.copy(srv.T)
        for k, v in vars(srv.T).items():
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(s.T, k, v.double())
        for k, v in vars(srv).items():
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(s, k, v.double())
        out.append(s)
    return out


@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def interpenetration(oracle, inp, pen_idx, cond_zero=False, dtype=torch.float64, vertex_path=True, warp_path=True, servers=None,
                     persons=None):
    """-> dict(loss (1,) with its graph, pairs {(a, b): dict(probe fields, s (m,), loss, active (m,) bool)}) over the ordered pairs of
    `persons` (default: all), keyed by POSITION in that list.  pen_idx {person: vertex ids}; inp carries smpl_params / smpl_pose /
    smpl_trans / smpl_shape (1,P,.), which may require grad.  vertex_path / warp_path: keep only that path of the gradient."""
    servers = oracle.servers if servers is None else servers
    persons = list(range(len(servers))) if persons is None else list(persons)
    scale = inp["smpl_params"][0, :, 0]
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in oracle.sd.items()}
    pv, tfs = {}, {}
    for p in persons:
        so = servers[p].forward(scale[p], inp["smpl_trans"][0, p], inp["smpl_pose"][0, p], inp["smpl_shape"][0, p])
        pv[p], tfs[p] = so["smpl_verts"].reshape(-1, 3).to(dtype), so["smpl_tfs"].reshape(24, 4, 4).to(dtype)
    total = torch.zeros(1, dtype=dtype)
    pairs = {}
    for a, p in enumerate(persons):
        x = pv[p][pen_idx[p].long()]
        if not vertex_path:
            x = x.detach()
        for b, q in enumerate(persons):
            if a == b:
                continue
            t = tfs[q] if warp_path else tfs[q].detach()
            r = probe(x, pv[q].detach(), t, oracle.persons[q].server.weights.to(dtype))
            cond = inp["smpl_pose"][0, q, 3:].detach().to(dtype) / np.pi
            if cond_zero:
                cond = torch.zeros_like(cond)
            s = O.implicit_forward(sd, oracle.persons[q].imp, r["xc"], cond, multires=6)[:, 0] if r["ids"].numel() else r["xc"][:, 0]
            active = s < 0
            loss = (s[active] ** 2).sum()
            total = total + loss
            pairs[(a, b)] = dict(r, s=s, active=active, loss=loss)
    return dict(loss=total, pairs=pairs)


def excluded_ok(pair):
    """the cap on a pair's excluded points: at most 0.5 % of its probed points and at most 8"""
    k = int(pair["excluded"].sum())
    return k <= EXCLUDED_MAX and k <= EXCLUDED_MAX_FRACTION * int(pair["probed"].sum())
