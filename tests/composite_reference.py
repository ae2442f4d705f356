"""Float64 reference of mp_composite and mp_tr_composite_bwd (include/multiply_hip.h), written from the header's definitions and
the reference's lines (multiply.py:425-480, 544-545, 590), not from the kernels: per ray the persons' samples are concatenated,
actually sorted by the key (t_end, person), and cumulative sums run along that list.  No rank lookups, no per-person prefix sums.

  composite_reference   numpy: every forward output, plus per ray the total free energy
  composite_outputs     the same in torch (float64 when given float64): the three outputs that have an adjoint
  autograd_gradients    float64 autograd into sdf[p], rgb[p], bg_rgb and beta (also per ray: every ray has a beta leaf of its own)
  adjoint_formulas      the second, independent statement: a numpy evaluation of the closed-form adjoint in the comment above
                        k_composite_bwd (compared with autograd in tests/test_composite_reference_cpu.py)

`mutate` re-states four mistakes an implementation could make; the CPU test measures what each one changes in float64 on the
committed cases, which is the argument that the device tests would see it:
  "last_gt"         the last sample on a tie of the final depths is the LOWER person's (last_sample with > instead of >=)
  "no_exception"    T_bg's adjoint also reaches the very last sample
  "inclusive_last"  T_bg includes the last sample's own free energy (pf[S] for the last person)
  "ignore_bg"       the background colour is taken as white"""
import functools

import numpy as np
import torch

from tests import geometry_reference as G
from tests import geometry_train_reference as GT

UP_KEYS = ("rgb_values", "acc", "acc_person")
MUTATIONS = ("last_gt", "no_exception", "inclusive_last", "ignore_bg")

# ---------------------------------------------------------------------------------------------------------------- cases
# (name, (R, P, n_z), beta, regime, seed of the inputs, seed of the colours and upstream gradients).  The shapes and betas are the
# siblings' (geometry_train_reference.CASES); "thin" draws sdf mostly positive so that the background shows through the hit rays.
# The seeds are chosen so that |d beta| >= 0.1 sum_rays |the ray's own d beta| (asserted on the CPU).
CASES = [
    ("opaque-70x3", (70, 3, 98), 0.1, "opaque", 4, 208),      # RAGGED_HITS: rays hit by 0 / 1 / 2 / 3 persons; S = 97: two passes
    ("opaque-70x3-sharp", (70, 3, 98), 0.02, "opaque", 4, 208),
    ("opaque-5x1", (5, 1, 65), 0.001, "opaque", 4, 208),      # S = 64: exactly one pass; sdf partly within a few beta (below)
    ("opaque-9x2", (9, 2, 34), 0.02, "opaque", 4, 208),       # S = 33: below one pass
    ("opaque-13x8", (13, 8, 130), 0.1, "opaque", 4, 208),     # the person limit, three passes
    ("thin-70x3", (70, 3, 98), 0.1, "thin", 4, 208),
    ("thin-5x1", (5, 1, 65), 0.1, "thin", 4, 208),
    ("thin-9x2", (9, 2, 34), 0.1, "thin", 4, 208),
    ("thin-13x8", (13, 8, 130), 0.1, "thin", 4, 208),
    ("tiny-6x2-thin", (6, 2, 2), 0.1, "thin", 4, 208),        # S = 1: the first sample is the last
    ("tiny-6x2-opaque", (6, 2, 2), 0.02, "opaque", 4, 208),
    ("tiny-6x3-thin", (6, 3, 3), 0.1, "thin", 4, 208),
    ("tiny-6x3-opaque", (6, 3, 3), 0.02, "opaque", 4, 208),
]
# the adjoint's adaptive launch shape at P = 8: 5S+2 floats per person fit 160 KiB of LDS with 4 waves up to S = 255, with 2 up to
# S = 511; the forward's fixed 4 waves of 3S+1 floats refuse from S = 427
LAUNCH_CASES = [
    ("launch-5x8x258", (5, 8, 258), 0.1, "thin", 4, 200),     # S = 257: 2 waves per block, an odd ray count
    ("launch-3x8x514", (3, 8, 514), 0.1, "thin", 4, 208),     # S = 513: 1 wave per block; the forward returns -2
]
THIN = [c for c in CASES if c[3] == "thin"]
BY_NAME = {c[0]: c for c in CASES + LAUNCH_CASES}


def _thin_sdf(rs, rows, S, P, beta):
    """sdf = off + N(0, 0.05) with off such that P persons of density sigma(off) over a ray of length 2 hold a free energy of
    about 1 (0.5 / beta exp(-off / beta) 2 P = 1), and two samples per row inside the surface (from S = 8 on).  With one or two
    samples per person the last sample, which T_bg leaves out, is all or half of a person: a denser draw (off - 0.18, off - 0.1)"""
    off = beta * np.log(P / beta) - (0.18 if S == 1 else 0.1 if S < 8 else 0.0)
    sdf = off + rs.randn(rows, S) * 0.05
    if S >= 8:
        for k in range(rows):
            j = rs.choice(S, 2, replace=False)
            sdf[k, j] = -np.abs(rs.randn(2)) * 0.02
    return sdf.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict of float32 numpy inputs: inv, z, sdf (G.ragged_case on GT.case_hits), rgb in [0,1], unit normals, bg in [0,1], and
    the upstream gradients up = {rgb_values (R,3), acc (R,), acc_person (R,P)} ~ N(0,1); shape, beta.  Leave it unchanged."""
    _, shape, beta, regime, seed, up_seed = BY_NAME[name]
    R, P, NZ = shape
    S = NZ - 1
    hits = [np.asarray(h, dtype=np.int64) for h in GT.case_hits(R, P)]     # (a person nobody hits keeps one row no ray refers to)
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=seed, hits=hits)
    rs = np.random.RandomState(1000 + seed)
    if regime == "thin":
        sdf = [_thin_sdf(rs, s.shape[0], S, P, beta) for s in sdf]
    elif beta < 0.01:
        # N(0, 0.05) alone leaves every sample saturated at beta = 0.001 and the gradient at 1e-9: half of the samples within
        # a few beta of the surface
        sdf = [np.where(rs.rand(*s.shape) < 0.5, rs.randn(*s.shape) * 3.0 * beta, s).astype(np.float32) for s in sdf]
    ru = np.random.RandomState(up_seed)
    rgb = [ru.rand(s.shape[0], S, 3).astype(np.float32) for s in sdf]
    nrm = [ru.randn(s.shape[0], S, 3) for s in sdf]
    nrm = [(n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32) for n in nrm]
    bg = ru.rand(R, 3).astype(np.float32)
    up = dict(rgb_values=ru.randn(R, 3).astype(np.float32), acc=ru.randn(R).astype(np.float32),
              acc_person=ru.randn(R, P).astype(np.float32))
    return dict(name=name, shape=shape, beta=beta, regime=regime, inv=inv, z=z, sdf=sdf, rgb=rgb, nrm=nrm, bg=bg, up=up)


# ---------------------------------------------------------------------------------------------------------------- forward
def _sort_key(te, who, person_sign):
    return sorted(range(len(te)), key=lambda j: (float(te[j]), person_sign * int(who[j])))


def composite_reference(n_rays, inv_index, z, sdf, rgb, normal, beta, bg_rgb=None, person_sign=1, mutate=None):
    """inv_index[n] (R,) int, z[n] (R_n, S+1), sdf[n] (R_n, S), rgb[n] / normal[n] (R_n, S, 3) for the P composited persons in column
    order; bg_rgb (R, 3) or None (white).  person_sign = -1 sorts ties of t_end with the HIGHER person first (the other tie rule).
    -> dict of float64: rgb_values, fg_rgb_values, normal_values (R,3), acc, bg_T, total (R,), acc_person (R,P).
    Colours and normals of samples whose weight is exactly 0 are never read (they may be NaN)."""
    assert mutate in (None,) + MUTATIONS
    P, R = len(inv_index), int(n_rays)
    beta = float(np.float32(beta))
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    z = [np.asarray(a, dtype=np.float64) for a in z]
    sdf = [np.asarray(a, dtype=np.float64) for a in sdf]
    rgb = [np.asarray(a, dtype=np.float64).reshape(len(s), -1, 3) for a, s in zip(rgb, sdf)]
    normal = [np.asarray(a, dtype=np.float64).reshape(len(s), -1, 3) for a, s in zip(normal, sdf)]
    bg = np.ones((R, 3)) if bg_rgb is None or mutate == "ignore_bg" else np.asarray(bg_rgb, dtype=np.float64)
    o = dict(rgb_values=np.zeros((R, 3)), fg_rgb_values=np.zeros((R, 3)), normal_values=np.zeros((R, 3)), acc=np.zeros(R),
             bg_T=np.ones(R), total=np.zeros(R), acc_person=np.zeros((R, P)))
    for r in range(R):
        ps = [n for n in range(P) if inv[n][r] >= 0]
        fg = np.zeros(3)
        if ps:
            te = np.concatenate([z[n][inv[n][r], 1:] for n in ps])
            fe = np.concatenate([G.laplace_density(sdf[n][inv[n][r]], beta) * np.diff(z[n][inv[n][r]]) for n in ps])
            who = np.concatenate([np.full(sdf[n].shape[1], n) for n in ps])
            c = np.concatenate([rgb[n][inv[n][r]] for n in ps])
            nv = np.concatenate([normal[n][inv[n][r]] for n in ps])
            order = _sort_key(te, who, person_sign)
            te, fe, who, c, nv = te[order], fe[order], who[order], c[order], nv[order]
            E = np.cumsum(fe) - fe                                        # free energy in front of every sample
            w = (1.0 - np.exp(-fe)) * np.exp(-E)
            live = w != 0
            fg = (w[live, None] * c[live]).sum(0)
            o["normal_values"][r] = (w[live, None] * nv[live]).sum(0)
            o["acc"][r], o["total"][r] = w.sum(), fe.sum()
            for n in ps:
                o["acc_person"][r, n] = w[who == n].sum()
            last = len(te) - 1                                            # the last element of the sorted list
            if mutate == "last_gt":                                       # the first of the persons that end at the final depth
                last = max(j for j in range(len(te)) if who[j] == min(who[te == te[-1]]))
            o["bg_T"][r] = np.exp(-(fe.sum() - (0.0 if mutate == "inclusive_last" else fe[last])))
        o["rgb_values"][r] = fg + o["bg_T"][r] * bg[r]
        o["fg_rgb_values"][r] = fg + o["bg_T"][r]
    return o


def composite_outputs(n_rays, inv_index, z, sdf, rgb, beta_rays, bg_rgb=None, person_sign=1):
    """torch restatement of the three outputs that have an adjoint.  z[n] (R_n, S+1), sdf[n] (R_n, S), rgb[n] (R_n, S, 3) tensors,
    beta_rays (R,) (ray r reads its own entry), bg_rgb (R, 3) or None -> {rgb_values (R,3), acc (R,), acc_person (R,P)}"""
    P, R = len(inv_index), int(n_rays)
    dt = z[0].dtype
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    zero = torch.zeros((), dtype=dt)
    rows = {k: [] for k in UP_KEYS}
    for r in range(R):
        ps = [n for n in range(P) if inv[n][r] >= 0]
        bg = torch.ones(3, dtype=dt) if bg_rgb is None else bg_rgb[r]
        cols = [zero] * P
        if not ps:
            rows["rgb_values"].append(1.0 * bg)
            rows["acc"].append(zero)
            rows["acc_person"].append(torch.stack(cols))
            continue
        te = torch.cat([z[n][inv[n][r], 1:] for n in ps])
        fe = torch.cat([GT.laplace_density(sdf[n][inv[n][r]], beta_rays[r]) * (z[n][inv[n][r], 1:] - z[n][inv[n][r], :-1]) for n in ps])
        who = torch.cat([torch.full((sdf[n].shape[1],), n, dtype=torch.long) for n in ps])
        c = torch.cat([rgb[n][inv[n][r]] for n in ps])
        idx = torch.tensor(_sort_key(te.detach().numpy(), who.numpy(), person_sign), dtype=torch.long)
        te, fe, who, c = te[idx], fe[idx], who[idx], c[idx]
        E = torch.cumsum(fe, 0) - fe
        w = (1.0 - torch.exp(-fe)) * torch.exp(-E)
        bg_T = torch.exp(-(fe.sum() - fe[-1]))                            # exclusive transmittance of the last element
        rows["rgb_values"].append((w[:, None] * c).sum(0) + bg_T * bg)
        rows["acc"].append(w.sum())
        for n in ps:
            cols[n] = w[who == n].sum()
        rows["acc_person"].append(torch.stack(cols))
    return {k: torch.stack(v) for k, v in rows.items()}


# ---------------------------------------------------------------------------------------------------------------- adjoint
def autograd_gradients(n_rays, inv_index, z, sdf, rgb, beta, bg_rgb, up, person_sign=1):
    """float64 autograd of sum_k <up[k], composite_outputs[k]>; up: {key of UP_KEYS: upstream gradient or None}.
    -> dict: d_sdf (list of (R_n, S)), d_rgb (list of (R_n, S, 3)), d_bg_rgb ((R,3), None without bg_rgb), d_beta (float),
    d_beta_rays ((R,): every ray's own part)"""
    R = int(n_rays)
    t64 = lambda a, g=False: torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=g)
    zt = [t64(a) for a in z]
    st = [t64(a, True) for a in sdf]
    ct = [t64(np.asarray(a).reshape(len(s), -1, 3), True) for a, s in zip(rgb, sdf)]
    bt = torch.full((R,), float(np.float32(beta)), dtype=torch.float64, requires_grad=True)
    gt = None if bg_rgb is None else t64(bg_rgb, True)
    out = composite_outputs(R, inv_index, zt, st, ct, bt, gt, person_sign)
    loss = bt.sum() * 0.0 + sum(s.sum() * 0.0 for s in st) + sum(c.sum() * 0.0 for c in ct) + (0.0 if gt is None else gt.sum() * 0.0)
    for k in UP_KEYS:
        if up.get(k) is not None:
            loss = loss + (t64(up[k]) * out[k]).sum()
    loss.backward()
    return dict(d_sdf=[s.grad.numpy() for s in st], d_rgb=[c.grad.numpy() for c in ct],
                d_bg_rgb=None if gt is None else gt.grad.numpy(), d_beta=float(bt.grad.sum()), d_beta_rays=bt.grad.numpy())


def adjoint_formulas(n_rays, inv_index, z, sdf, rgb, beta, bg_rgb, up, person_sign=1, mutate=None):
    """float64 numpy evaluation of the closed-form adjoint: with dC / dA / dA_p the ray's upstream gradients of rgb_values / acc /
    acc_person, dw_j = dC . rgb_j + dA + dA_p(j), dT_bg = dC . bg, in merged order
        d fe_j = dw_j T_j exp(-fe_j) - sum_{i behind j} dw_i w_i - [j is not the very last sample] dT_bg T_bg
        d rgb_j = w_j dC,   d bg = T_bg dC,   d sigma_j = d fe_j (te - ts)_j -> d sdf, d beta through the Laplace density.
    -> the dict of autograd_gradients"""
    assert mutate in (None,) + MUTATIONS
    P, R = len(inv_index), int(n_rays)
    beta = float(np.float32(beta))
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    z = [np.asarray(a, dtype=np.float64) for a in z]
    sdf = [np.asarray(a, dtype=np.float64) for a in sdf]
    rgb = [np.asarray(a, dtype=np.float64).reshape(len(s), -1, 3) for a, s in zip(rgb, sdf)]
    g = {k: (None if up.get(k) is None else np.asarray(up[k], dtype=np.float64)) for k in UP_KEYS}
    white = bg_rgb is None or mutate == "ignore_bg"
    bg = np.ones((R, 3)) if white else np.asarray(bg_rgb, dtype=np.float64)
    d_sdf, d_rgb = [np.zeros_like(s) for s in sdf], [np.zeros_like(c) for c in rgb]
    d_bg, d_beta_rays = np.zeros((R, 3)), np.zeros(R)
    for r in range(R):
        dC = np.zeros(3) if g["rgb_values"] is None else g["rgb_values"][r]
        dA = 0.0 if g["acc"] is None else float(g["acc"][r])
        ps = [n for n in range(P) if inv[n][r] >= 0]
        if not ps:
            d_bg[r] = dC
            continue
        key = [(z[n][inv[n][r], i + 1], n, i) for n in ps for i in range(sdf[n].shape[1])]
        key.sort(key=lambda a: (a[0], person_sign * a[1], a[2]))
        m_n, m_i = np.array([a[1] for a in key]), np.array([a[2] for a in key])
        rows = inv_rows = np.array([inv[n][r] for n in m_n])
        m_dt = np.array([z[n][k, i + 1] - z[n][k, i] for n, k, i in zip(m_n, rows, m_i)])
        m_s = np.array([sdf[n][k, i] for n, k, i in zip(m_n, rows, m_i)])
        m_c = np.stack([rgb[n][k, i] for n, k, i in zip(m_n, rows, m_i)])
        fe = G.laplace_density(m_s, beta) * m_dt
        E = np.cumsum(fe) - fe
        T = np.exp(-E)
        w = (1 - np.exp(-fe)) * T
        dAp = np.zeros(len(fe)) if g["acc_person"] is None else g["acc_person"][r][m_n]
        dw = m_c @ dC + dA + dAp
        behind = np.cumsum((dw * w)[::-1])[::-1] - dw * w
        last = len(fe) - 1
        if mutate == "last_gt":
            last = max(j for j in range(len(fe)) if m_n[j] == min(m_n[np.array([a[0] for a in key]) == key[-1][0]]))
        Tbg = np.exp(-(fe.sum() - (0.0 if mutate == "inclusive_last" else fe[last])))
        dTbg = float(dC @ bg[r])
        dfe = dw * T * np.exp(-fe) - behind - dTbg * Tbg
        if mutate not in ("no_exception", "inclusive_last"):
            dfe[last] += dTbg * Tbg
        d_bg[r] = dC * Tbg
        dsig = dfe * m_dt
        eab = np.exp(-np.abs(m_s) / beta)
        dbe = np.where(m_s > 0, 0.5 / beta**2 * eab * (m_s / beta - 1),
                       np.where(m_s < 0, -1 / beta**2 + 0.5 / beta**2 * eab * (1 + m_s / beta), -0.5 / beta**2))
        dsd = dsig * (-(0.5 / beta**2) * eab)
        for a, (n, k, i) in enumerate(zip(m_n, inv_rows, m_i)):
            d_sdf[n][k, i] += dsd[a]
            d_rgb[n][k, i] += w[a] * dC
        d_beta_rays[r] = float((dsig * dbe).sum())
    return dict(d_sdf=d_sdf, d_rgb=d_rgb, d_bg_rgb=None if bg_rgb is None else d_bg, d_beta=float(d_beta_rays.sum()),
                d_beta_rays=d_beta_rays)


@functools.lru_cache(maxsize=None)
def reference(name, only=None, white=False):
    """the case's float64 forward and autograd gradients (all three upstream gradients, or the one named `only`; white: bg_rgb
    is None), computed once and shared: leave it unchanged.  -> (case dict, forward dict, gradient dict, the upstream dict used)"""
    c = case(name)
    bg = None if white else c["bg"]
    up = {k: (v if only in (None, k) else None) for k, v in c["up"].items()}
    fwd = composite_reference(c["shape"][0], c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], bg)
    grad = autograd_gradients(c["shape"][0], c["inv"], c["z"], c["sdf"], c["rgb"], c["beta"], bg, up)
    return c, fwd, grad, up


def last_samples(inv_index, sdf):
    """per person a mask (R_n, S) of the last sample of every row that a ray refers to"""
    out = []
    for iv, s in zip(inv_index, sdf):
        m = np.zeros(s.shape, bool)
        iv = np.asarray(iv)
        m[iv[iv >= 0], -1] = True
        out.append(m)
    return out


def thin_subset(inv_index, sdf, bg_T, floor=0.05):
    """the restricted measure of the thin cases: per person a mask (R_n, S) of the last sample of every person on every ray and
    of all samples of the rays with bg_T >= floor"""
    out = last_samples(inv_index, sdf)
    for m, iv in zip(out, inv_index):
        iv = np.asarray(iv)
        m[iv[(iv >= 0) & (np.asarray(bg_T) >= floor)]] = True
    return out


def _all(want, masks):
    return [np.ones(w.shape, bool) for w in want] if masks is None else masks


def top_of(want, masks=None):
    """max |want| over the samples of `masks` (default: all)"""
    return max([float(np.abs(w[m]).max()) for w, m in zip(want, _all(want, masks)) if m.any()], default=0.0)


def abs_error(got, want, masks=None):
    """max |got - want| over the samples of `masks` (default: all)"""
    return max([float(np.abs(np.asarray(g, dtype=np.float64)[m] - w[m]).max()) for g, w, m in zip(got, want, _all(want, masks)) if m.any()],
               default=0.0)


def dsdf_error(got, want, masks=None):
    """max |got - want| over max |want|, both over the samples of `masks` -> (ratio, the scale)"""
    top = top_of(want, masks)
    return (abs_error(got, want, masks) / top if top > 0 else float("inf")), top


# ---------------------------------------------------------------------------------------------------------------- constructed rows
def tied_rows():
    """(a) two persons with identical depth rows: every t_end ties, the lower column goes first.  Thin, so that the order shows
    in every output.  -> case-like dict (R = 7, P = 2, n_z = 98, beta = 0.1)"""
    R, P, NZ, beta = 7, 2, 98, 0.1
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=11)
    z[1] = z[0].copy()
    rs = np.random.RandomState(1011)
    sdf = [_thin_sdf(rs, R, NZ - 1, P, beta) for _ in range(P)]
    return _dress(dict(name="tied rows", shape=(R, P, NZ), beta=beta, inv=inv, z=z, sdf=sdf), 211)


def last_tie_rows():
    """(b) the last-sample tie: thin rays on which the final depths of both persons are equal.  Rays 0..2: person 0's last sample
    is dense (sdf = -1), person 1's thin; rays 3..5: the mirror image; ray 6: person 0 ends behind person 1 (no tie: person 0's
    last sample is the last of the list); ray 7: person 1 ends behind person 0.  Only the final depths tie.
    -> case-like dict (R = 8, P = 2, n_z = 34, beta = 0.1)"""
    R, P, NZ, beta = 8, 2, 34, 0.1
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=13)
    rs = np.random.RandomState(1013)
    sdf = [(0.35 + rs.randn(R, NZ - 1) * 0.05).astype(np.float32) for _ in range(P)]
    for n in range(P):                                   # a last interval of length 0.1 .. 0.2, so that a dense last sample has fe ~ 1
        z[n][:, :-1] = np.minimum(z[n][:, :-1], np.float32(2.8))
        z[n][:, -1] = z[n][:, -2] + np.float32(0.1) * (1 + rs.rand(R).astype(np.float32))
    z[0][:6, -1] = z[1][:6, -1] = np.float32(3.0)
    z[0][6, -1], z[1][6, -1] = np.float32(3.0), np.float32(2.95)
    z[0][7, -1], z[1][7, -1] = np.float32(2.95), np.float32(3.0)
    sdf[0][:3, -1], sdf[1][3:6, -1] = -1.0, -1.0
    sdf[0][6, -1], sdf[1][7, -1] = -1.0, -1.0
    for n in range(P):
        assert (np.diff(z[n], axis=1) >= 0).all()
    return _dress(dict(name="last-sample tie", shape=(R, P, NZ), beta=beta, inv=inv, z=z, sdf=sdf), 213)


def zero_weight_rows():
    """(c) at beta = 0.001, where sdf = +1 has exactly no density: ray 0 empty for both persons; ray 1: person 0's first sample
    is opaque, every later weight underflows to exactly 0; ray 2: repeated depths (dt = 0) among dense samples; the other rays as
    drawn.  Colours AND normals of every sample with fe == 0 are NaN.  -> case-like dict (R = 7, P = 2, n_z = 34, beta = 0.001)"""
    R, P, NZ, beta = 7, 2, 34, 0.001
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=12)
    grid = (1.0 + 0.05 * np.arange(NZ)).astype(np.float32)
    sdf[0][0], sdf[1][0] = 1.0, 1.0
    z[0][1] = (1.0 + 0.2 * np.arange(NZ)).astype(np.float32)   # fe = 200 in sample 0: exp(-200) is 0 in float32
    sdf[0][1], sdf[1][1] = 1.0, 1.0
    sdf[0][1, 0::2] = -1.0                               # behind it dense samples (finite colours, weight 0 in float32) and empty ones
    sdf[1][1, (NZ - 1) // 2:] = -1.0
    z[0][2], z[1][2] = grid.copy(), grid + np.float32(0.02)
    z[0][2, 9:12] = z[0][2, 8]                           # samples 8..10 of person 0 have dt = 0
    sdf[0][2], sdf[1][2] = 1.0, 1.0
    sdf[0][2, 6:13] = np.float32(0.004)                  # density 1/beta * 0.5 e^-4 = 9.2: fe = 0.46 where dt = 0.05, 0 where dt = 0
    sdf[1][3:, ::2] = 1.0                                # the drawn rays: every other sample of person 1 is empty
    c = _dress(dict(name="zero weights", shape=(R, P, NZ), beta=beta, inv=inv, z=z, sdf=sdf), 212)
    for n in range(P):
        fe = G.laplace_density(c["sdf"][n].astype(np.float64), float(np.float32(beta))) * np.diff(c["z"][n].astype(np.float64), axis=1)
        c["rgb"][n][fe == 0] = np.nan
        c["nrm"][n][fe == 0] = np.nan
    return c


def _dress(c, seed):
    """colours, unit normals, background and upstream gradients for constructed rows"""
    R, P, NZ = c["shape"]
    ru = np.random.RandomState(seed)
    c["rgb"] = [ru.rand(s.shape[0], NZ - 1, 3).astype(np.float32) for s in c["sdf"]]
    nrm = [ru.randn(s.shape[0], NZ - 1, 3) for s in c["sdf"]]
    c["nrm"] = [(n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32) for n in nrm]
    c["bg"] = ru.rand(R, 3).astype(np.float32)
    c["up"] = dict(rgb_values=ru.randn(R, 3).astype(np.float32), acc=ru.randn(R).astype(np.float32),
                   acc_person=ru.randn(R, P).astype(np.float32))
    return c
