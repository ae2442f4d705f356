"""Float64 numpy restatement of the registration (multiply_amd/registration.py, csrc/registration.hip, csrc/reg_solve.hpp): the
rows of the point-to-plane normal equations, the Gauss-Newton step, Umeyama's closed form and the ICP loop.  The reference project
has no such code; the definitions are those of include/multiply_hip.h, restated independently (numpy.linalg for the solve and the
SVD).  The closest query is mesh_metrics_reference.closest.  tests/test_registration_cpu.py pins this file before anything on the
device is compared against it."""
import numpy as np

from tests import mesh_metrics_reference as MR

# the state block and the slot (include/multiply_hip.h MP_REG_*)
STATE, SLOT = 32, 40
S, R, T, TAU2, RMS, ACCEPTED, REJECTED, LEFT_OUT, ITERS, FLAG, STEP, C, BOX_LO, BOX_HI, RMS_PLANE = 0, 1, 10, 13, 14, 15, 16, 17, 18, 19, \
    20, 21, 24, 27, 30
ATA, ATR, R2, D2, N_ACC, N_REJ, N_OUT = 0, 28, 35, 36, 37, 38, 39
CONVERGED, DEGENERATE = 1, 2
TRIU = np.triu_indices(7)


def new_state(scale, Rm, t, lo, hi, tau2=np.inf):
    st = np.zeros(STATE)
    st[S], st[R:R + 9], st[T:T + 3], st[TAU2] = scale, np.asarray(Rm, np.float64).reshape(9), t, tau2
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    st[C:C + 3], st[BOX_LO:BOX_LO + 3], st[BOX_HI:BOX_HI + 3] = 0.5 * (lo + hi), lo, hi
    return st


def transform(st):
    return st[S], st[R:R + 9].reshape(3, 3), st[T:T + 3]


def apply(st, p, inverse=False):
    s, Rm, t = transform(st)
    p = np.asarray(p, np.float64)
    return ((p - t) @ Rm) / s if inverse else s * (p @ Rm.T) + t


def rows(p, q, normals, st, in_source=False, face=None, mask=None):
    """one direction's slot (SLOT,), the mask (0 accepted / 1 rejected / 2 left out) and the per-pair terms (n, SLOT) it sums.
    mask: take this accept decision (a device's own) instead of deciding here"""
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    n = p.shape[0]
    if face is not None:
        face = np.asarray(face)
        ok = (face >= 0) & (face < nrm.shape[0])
        nrm = np.where(ok[:, None], nrm[np.where(ok, face, 0)], np.nan)
    s, Rm, t = transform(st)
    with np.errstate(all="ignore"):
        if in_source:
            nrm = nrm @ Rm.T
        x = s * (p @ Rm.T) + t
        e = x - q
        d2 = (e * e).sum(1)
        fin = np.isfinite(d2) & np.isfinite(nrm).all(1)
        rej = fin & (d2 > st[TAU2])
        if mask is not None:
            fin, rej = np.asarray(mask) != 2, np.asarray(mask) == 1
        acc = fin & ~rej
        xc = x - st[C:C + 3]
        a = np.concatenate([np.cross(xc, nrm), nrm, (xc * nrm).sum(1, keepdims=True)], 1)
        r = (e * nrm).sum(1)
        terms = np.zeros((n, SLOT))
        terms[:, ATA:ATA + 28] = (a[:, :, None] * a[:, None, :])[:, TRIU[0], TRIU[1]]
        terms[:, ATR:ATR + 7] = a * r[:, None]
        terms[:, R2], terms[:, D2], terms[:, N_ACC] = r * r, d2, 1.0
        terms = np.where(acc[:, None], terms, 0.0)
    terms[:, N_REJ], terms[:, N_OUT] = rej, ~fin
    mask = np.where(acc, 0, np.where(rej, 1, 2)).astype(np.uint8)
    return terms.sum(0), mask, terms


def rodrigues(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def normal_matrix(sums, m):
    A = np.zeros((7, 7))
    A[TRIU] = sums[ATA:ATA + 28]
    A = A + np.triu(A, 1).T
    return A[:m, :m], -sums[ATR:ATR + m]


def sums_from(A, b, n_acc=100.0):
    """a summed slot whose normal equations are A delta = b (A (7,7) symmetric, b = -A^T r), with n_acc accepted pairs"""
    s = np.zeros(SLOT)
    s[ATA:ATA + 28] = A[TRIU]
    s[ATR:ATR + 7] = -b
    s[R2], s[D2], s[N_ACC] = 1e-4 * n_acc, 4e-4 * n_acc, n_acc
    return s


def step(sums, st, similarity, reject=3.0, tol=1e-6):
    """the state after one Gauss-Newton step from the summed slot, and delta (7,) (None when degenerate)"""
    st = st.copy()
    if st[FLAG] != 0:
        return st, None
    acc = sums[N_ACC]
    st[ACCEPTED], st[REJECTED], st[LEFT_OUT] = acc, sums[N_REJ], sums[N_OUT]
    st[RMS] = np.sqrt(sums[D2] / acc) if acc > 0 else 0.0
    st[RMS_PLANE] = np.sqrt(sums[R2] / acc) if acc > 0 else 0.0
    m = 7 if similarity else 6
    A, b = normal_matrix(sums, m)
    ok = acc >= 7
    if ok:
        try:
            np.linalg.cholesky(A)
            ok = np.linalg.cond(A / np.sqrt(np.outer(np.diag(A), np.diag(A)))) < 1e11
        except np.linalg.LinAlgError:
            ok = False
    if not ok:
        st[FLAG], st[STEP] = DEGENERATE, 0.0
        return st, None
    d = np.zeros(7)
    d[:m] = np.linalg.solve(A, b)
    s, Rm, t = transform(st)
    E, es, c = rodrigues(d[:3]), np.exp(d[6]), st[C:C + 3]
    new = st.copy()
    new[S], new[R:R + 9], new[T:T + 3] = s * es, (E @ Rm).reshape(9), c + es * (E @ (t - c)) + d[3:6]
    lo, hi = st[BOX_LO:BOX_LO + 3], st[BOX_HI:BOX_HI + 3]
    corners = np.array([[hi[a] if (k >> a) & 1 else lo[a] for a in range(3)] for k in range(8)])
    size = np.linalg.norm(apply(new, corners) - apply(st, corners), axis=1).max()
    new[TAU2] = (reject * st[RMS]) ** 2 if reject > 0 else np.inf
    new[ITERS], new[STEP] = st[ITERS] + 1, size
    if size <= tol * np.linalg.norm(hi - lo):
        new[FLAG] = CONVERGED
    return new, d


def umeyama(p, q, w=None, similarity=False):
    """(s, R, t) minimising sum w |s R p + t - q|^2 (Umeyama 1991): numpy SVD, det-corrected; and the singular values"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    w = np.ones(p.shape[0]) if w is None else np.asarray(w, np.float64)
    sw = w.sum()
    pm, qm = (w[:, None] * p).sum(0) / sw, (w[:, None] * q).sum(0) / sw
    pc, qc = p - pm, q - qm
    H = (w[:, None, None] * pc[:, :, None] * qc[:, None, :]).sum(0)          # row = p axis, column = q axis
    U, Sg, Vt = np.linalg.svd(H)
    V, D = Vt.T, np.ones(3)
    if np.linalg.det(V @ U.T) < 0:
        D[2] = -1.0
    Rm = V @ np.diag(D) @ U.T
    s = (Sg * D).sum() / (w * (pc * pc).sum(1)).sum() if similarity else 1.0
    return s, Rm, qm - s * Rm @ pm, Sg, D


def icp(src, dst, ps, qs, similarity, max_iters=30, reject=3.0, tol=1e-6, init=None, history=None):
    """the loop of registration.register in float64 on GIVEN samples ps (on src) and qs (on dst): src, dst = (vertices, faces);
    init = (s, R, t) (None: the centroid start).  Returns the final state."""
    (sv, sf), (dv, df) = [(np.asarray(v, np.float64), np.asarray(f)) for v, f in (src, dst)]
    sfv, dfv = sv[sf], dv[df]
    sn, dn = MR.face_normals(sfv), MR.face_normals(dfv)
    ps, qs = np.asarray(ps, np.float64), np.asarray(qs, np.float64)
    if init is None:
        pm, qm = ps.mean(0), qs.mean(0)
        s0 = np.sqrt(((qs - qm) ** 2).sum(1).mean() / ((ps - pm) ** 2).sum(1).mean()) if similarity else 1.0
        init = (s0, np.eye(3), qm - s0 * pm)
    st = new_state(init[0], init[1], init[2], dv.min(0), dv.max(0))
    for _ in range(max_iters):
        _, f1, q1 = MR.closest(apply(st, ps), dfv)
        a = rows(ps, q1, dn, st, False, f1)[0]
        _, f2, p2 = MR.closest(apply(st, qs, inverse=True), sfv)
        b = rows(p2, qs, sn, st, True, f2)[0]
        st, _ = step(a + b, st, similarity, reject, tol)
        if history is not None:
            history.append(st.copy())
        if st[FLAG] != 0:
            break
    return st
