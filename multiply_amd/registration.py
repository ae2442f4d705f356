"""Registration of meshes before the mesh metrics: the rigid or similarity transform x = s R p + t that carries a reconstruction
into the frame of the ground truth it is judged against.

A monocular reconstruction lives in the normalised scene frame, with an unknown global scale and a rigid offset against the scans;
without alignment Chamfer, P2S, F-score and volume IoU measure that mismatch (metrics.mesh_metrics(align=...) calls this module).
The reference project ships no code for it.  Definitions:

  fit_pairs          the closed form for explicit pairs (Umeyama 1991; mp_reg_fit_pairs), e.g. a prediction's SMPL vertices against
                     the ground truth's, as an initial transform;
  register           point-to-plane ICP (Chen & Medioni 1992) on closest-SURFACE correspondences: per iteration and direction the
                     samples are carried over (mp_reg_apply), the exact closest face is queried (hip.mesh_closest, through a
                     MeshIndex or brute force: same bits), the pairs are reduced to the 7 x 7 normal equations (mp_reg_rows), and
                     one launch solves them and composes the update (mp_reg_step).  Source -> target pairs use the target's face
                     normals; target -> source pairs the source's, rotated into the target frame.  Pairs farther apart than
                     `reject` x the last RMS distance are rejected (all are accepted in the first iteration).  The whole state lives
                     in one device block (include/multiply_hip.h MP_REG_*); once it carries the converged or degenerate flag the
                     launches return at once, so the host reads it only every `check_every` iterations.  Both meshes are
                     sampled with ONE seeded set of uniforms, stratified over the area CDF (sample_uniforms);
  register_sequence  ONE transform for all frames of a sequence (two slots per frame, one step over all of them): with a static
                     camera the prediction-to-scan transform is a single similarity, and a per-frame alignment would hide
                     translation and pose errors.
  converged          the step size -- the largest displacement of the 8 corners of the target's bounding box between two
                     consecutive transforms -- is at most tol x the box's diagonal.

Point-to-plane, not point-to-point: on closest-surface pairs the latter contracts by a few per cent per iteration.
ICP is local: `init` must bring the meshes within the basin (centroids and, for a similarity, RMS radii by default).  Everything
heavy runs on the device; this module imports without one."""
import numpy as np
import torch

from . import hip

KINDS = ("rigid", "similarity")
DIRECTIONS = ("both", "forward", "backward")


class Similarity:
    """x = scale R p + t, float64 numpy: scale > 0, R (3,3) a rotation, t (3,)"""

    def __init__(self, scale=1.0, R=None, t=None):
        self.scale = float(scale)
        self.R = np.eye(3) if R is None else np.array(R, dtype=np.float64).reshape(3, 3)
        self.t = np.zeros(3) if t is None else np.array(t, dtype=np.float64).reshape(3)

    @classmethod
    def from_matrix(cls, M):
        M = np.asarray(M, np.float64)
        A = M[:3, :3]
        s = float(np.cbrt(np.linalg.det(A)))
        return cls(s, A / s, M[:3, 3])

    @property
    def matrix(self):
        M = np.eye(4)
        M[:3, :3] = self.scale * self.R
        M[:3, 3] = self.t
        return M

    def apply(self, points):
        """points (..., 3): a numpy array gives float64 numpy, a tensor gives a tensor of its dtype and device (computed in float64)"""
        if torch.is_tensor(points):
            R = torch.from_numpy(self.R).to(points.device)
            t = torch.from_numpy(self.t).to(points.device)
            return (self.scale * (points.double() @ R.T) + t).to(points.dtype)
        return self.scale * (np.asarray(points, np.float64) @ self.R.T) + self.t

    def inverse(self):
        return Similarity(1.0 / self.scale, self.R.T, -(self.R.T @ self.t) / self.scale)

    def compose(self, other):
        """self after other: (self.compose(other)).apply(p) = self.apply(other.apply(p))"""
        return Similarity(self.scale * other.scale, self.R @ other.R, self.scale * (self.R @ other.t) + self.t)

    def __repr__(self):
        return f"Similarity(scale={self.scale!r}, R={self.R.tolist()!r}, t={self.t.tolist()!r})"


def _kind(kind):
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    return kind


def fit_pairs(p, q, weights=None, kind="rigid", device="cuda"):
    """The Similarity minimising sum w |s R p + t - q|^2 over the pairs p, q (n,3) (numpy or tensors), s = 1 for kind 'rigid'.
    Pairs with a non-finite value or a weight that is not positive are left out."""
    sim = _kind(kind) == "similarity"
    dev = p.device if torch.is_tensor(p) and p.is_cuda else device
    as_t = lambda x: None if x is None else torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).detach().to(dev).float()
    p, q, w = as_t(p), as_t(q), as_t(weights)
    out = hip.reg_fit_pairs(p.reshape(-1, 3), q.reshape(-1, 3), None if w is None else w.reshape(-1), sim).cpu().numpy()
    if out[15] == 1.0:
        raise ValueError("fit_pairs: no pair with a positive weight and finite coordinates")
    return Similarity(out[0], out[1:10], out[10:13])


def state_similarity(state):
    """the Similarity in a state block (a device tensor or a numpy array)"""
    st = state.detach().cpu().numpy() if torch.is_tensor(state) else np.asarray(state)
    return Similarity(st[hip.REG_S], st[hip.REG_R:hip.REG_R + 9], st[hip.REG_T:hip.REG_T + 3])


def transform_vertices(verts, sim):
    """verts (n,3) float32 device tensor under the Similarity: mp_reg_apply (double arithmetic, rounded once)"""
    z = np.zeros(3)
    return hip.reg_apply(verts, hip.reg_state(sim.scale, sim.R, sim.t, z, z, verts.device))


def sample_uniforms(n, seed, device):
    """(n,3) uniforms for metrics.surface_samples from a device generator seeded with `seed`, as mesh_metrics draws them, except
    that the first column -- the one that picks the face through the area CDF -- is STRATIFIED: sample i draws from [i / n,
    (i + 1) / n).  Every face then gets its share of the samples by area to within one, instead of a binomial count.  Each sample
    is still uniform on the surface; what goes is the noise of uneven coverage, which on meshes that differ in tessellation
    dominates the estimate: the residual is a fixed field over the surface, and the fit integrates it (the spread
    of the result over sample sets falls from 1.2 % to 0.2 % of the surface RMS at 600 samples)."""
    n = int(n)
    u = torch.rand(n, 3, generator=torch.Generator(device=device).manual_seed(int(seed)), device=device)
    u0 = (torch.arange(n, device=device, dtype=torch.float64) + u[:, 0].double()) / n
    u[:, 0] = u0.float().clamp_(max=1.0 - 2.0 ** -24)
    return u


def _snapshot(st):
    flag = int(st[hip.REG_FLAG])
    return dict(iterations=int(st[hip.REG_ITERS]), rms=float(st[hip.REG_RMS]), rms_plane=float(st[hip.REG_RMS_PLANE]),
                step=float(st[hip.REG_STEP]), accepted=int(st[hip.REG_ACCEPTED]), rejected=int(st[hip.REG_REJECTED]),
                left_out=int(st[hip.REG_LEFT_OUT]), converged=flag == hip.REG_CONVERGED, degenerate=flag == hip.REG_DEGENERATE)


def _register(srcs, dsts, kind, n_samples, max_iters, reject, tol, init, directions, seed, index_mode, check_every, details):
    from .metrics import as_mesh, surface_samples
    sim = _kind(kind) == "similarity"
    if directions not in DIRECTIONS:
        raise ValueError(f"directions must be one of {DIRECTIONS}, got {directions!r}")
    if len(srcs) != len(dsts) or not srcs:
        raise ValueError("register_sequence needs as many source as target meshes, at least one")
    if int(n_samples) < 1 or int(max_iters) < 0 or int(check_every) < 1:
        raise ValueError("n_samples >= 1, max_iters >= 0 and check_every >= 1 are required")
    if not isinstance(init, Similarity) and init not in ("centroid", "identity"):
        raise ValueError(f"init must be 'centroid', 'identity' or a Similarity, got {init!r}")
    hip.mesh_index_mode(index_mode)
    hip.require_device()
    fwd, bwd = directions in ("both", "forward"), directions in ("both", "backward")
    frames, u = [], None
    for s_mesh, d_mesh in zip(srcs, dsts):
        fr = {}
        for side, mesh in (("src", s_mesh), ("dst", d_mesh)):
            v, f = as_mesh(mesh)
            if u is None:       # ONE seeded set of uniforms for every mesh
                u = sample_uniforms(n_samples, seed, v.device)
            fv = v[f].contiguous()
            pts, _, _ = surface_samples((v, f), n_samples, uniforms=u)
            fr[side] = dict(v=v, fv=fv, fn=hip.fit_area_cdf(fv)[1], pts=pts,
                            index=hip.MeshIndex(fv) if hip.mesh_index_wanted(index_mode, fv.shape[0], f) else None)
        frames.append(fr)
    dev = frames[0]["src"]["v"].device
    lo = torch.stack([fr["dst"]["v"].min(0).values for fr in frames]).min(0).values.double().cpu().numpy()
    hi = torch.stack([fr["dst"]["v"].max(0).values for fr in frames]).max(0).values.double().cpu().numpy()
    if isinstance(init, Similarity):
        T0 = init
    elif init == "identity":
        T0 = Similarity()
    else:
        P = torch.cat([fr["src"]["pts"] for fr in frames]).double()
        Q = torch.cat([fr["dst"]["pts"] for fr in frames]).double()
        P, Q = P[torch.isfinite(P).all(1)], Q[torch.isfinite(Q).all(1)]
        pm, qm = P.mean(0), Q.mean(0)
        s0 = 1.0
        if sim:
            rp, rq = float(((P - pm) ** 2).sum(1).mean().sqrt()), float(((Q - qm) ** 2).sum(1).mean().sqrt())
            s0 = rq / rp if rp > 0.0 and rq > 0.0 else 1.0
        T0 = Similarity(s0, np.eye(3), qm.cpu().numpy() - s0 * pm.cpu().numpy())
    state = hip.reg_state(T0.scale, T0.R, T0.t, lo, hi, dev)
    per = int(fwd) + int(bwd)
    slots = torch.zeros(per * len(frames), hip.REG_SLOT, dtype=torch.float64, device=dev)
    work = hip.reg_work(dev)
    x = torch.empty(int(n_samples), 3, dtype=torch.float32, device=dev)
    history, st = [], None
    if details is not None:
        details.update(frames=frames, init=T0, iterations=[])
    it = 0
    while it < int(max_iters):
        rec = None
        if details is not None:
            rec = dict(state_before=state.cpu().numpy().copy(), slots=[])
        j = 0
        for fr in frames:
            S, D = fr["src"], fr["dst"]
            if fwd:
                hip.reg_apply(S["pts"], state, out=x)
                _, face, q = hip.mesh_closest(x, D["fv"], index=D["index"])
                mask = torch.empty(x.shape[0], dtype=torch.uint8, device=dev) if rec is not None else None
                hip.reg_rows(S["pts"], q, D["fn"], state, slots[j], face=face, work=work, mask=mask)
                if rec is not None:
                    rec["slots"].append(dict(p=S["pts"], q=q, face=face, normals=D["fn"], normals_in_source=False, mask=mask))
                j += 1
            if bwd:
                hip.reg_apply(D["pts"], state, inverse=True, out=x)
                _, face, p = hip.mesh_closest(x, S["fv"], index=S["index"])
                mask = torch.empty(x.shape[0], dtype=torch.uint8, device=dev) if rec is not None else None
                hip.reg_rows(p, D["pts"], S["fn"], state, slots[j], face=face, normals_in_source=True, work=work, mask=mask)
                if rec is not None:
                    rec["slots"].append(dict(p=p, q=D["pts"], face=face, normals=S["fn"], normals_in_source=True, mask=mask))
                j += 1
        hip.reg_step(slots, state, similarity=sim, reject=reject, tol=tol)
        it += 1
        if rec is not None:
            rec.update(slot_sums=slots.cpu().numpy().copy(), state_after=state.cpu().numpy().copy())
            details["iterations"].append(rec)
        if it % int(check_every) == 0 or it == int(max_iters):
            st = state.cpu().numpy()
            history.append(_snapshot(st))
            if st[hip.REG_FLAG] != 0.0:
                break
    if st is None:
        st = state.cpu().numpy()
        history.append(_snapshot(st))
    info = _snapshot(st)
    info.update(kind=kind, history=history, n_samples=int(n_samples), n_frames=len(frames))
    if details is not None:
        details["state"] = st.copy()
    return state_similarity(st), info


def register(src, dst, kind="rigid", n_samples=20000, max_iters=30, reject=3.0, tol=1e-6, init="centroid", directions="both",
             seed=0, index_mode="auto", check_every=5, details=None):
    """(Similarity T, info) with T(src) aligned to dst; meshes as metrics.as_mesh accepts them.  info: rms (of the accepted
    point-to-point distances at the last step's start), rms_plane, iterations, converged, degenerate, accepted / rejected / left_out
    (pairs of the last step), step, history (one such record per read-back of the state: every check_every iterations and at the
    end; `iterations` is exact, the loop itself may have been launched up to check_every - 1 idle iterations further).  init:
    'centroid' (sample centroids; for a similarity also the ratio of the RMS radii; identity rotation), 'identity', or a Similarity.
    directions: 'both' | 'forward' (source samples only) | 'backward'.  details: a dict that receives the samples and, per
    iteration, the pairs, the accept masks and the state before and after (for tests; it synchronises every iteration)."""
    return _register([src], [dst], kind, n_samples, max_iters, reject, tol, init, directions, seed, index_mode, check_every, details)


def register_sequence(srcs, dsts, kind="similarity", n_samples=20000, max_iters=30, reject=3.0, tol=1e-6, init="centroid",
                      directions="both", seed=0, index_mode="auto", check_every=5, details=None):
    """ONE (Similarity, info) for all frames: srcs[k] is aligned to dsts[k] by the same transform.  n_samples per mesh and frame;
    the acceptance threshold and the convergence test are those of register over the union of the frames."""
    return _register(list(srcs), list(dsts), kind, n_samples, max_iters, reject, tol, init, directions, seed, index_mode, check_every,
                     details)
