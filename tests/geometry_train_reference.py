"""Differentiable restatement of mp_composite_geometry's five differentiable outputs (include/multiply_hip.h), written from the
header's definitions and not from the kernels: per ray the merged sample list is built by actually sorting the key
(t_end, person), then cumulative sums along it; a person's solo list is its own samples sorted the same way.  torch autograd
carries the gradient into sdf and beta (z is a constant); float64 when given float64.  The forward values are cross-checked
against tests/geometry_reference.py (tests/test_geometry_train_cpu.py).

`adjoint_formulas` is the second, independent statement the tests compare autograd with: a float64 numpy evaluation of the
closed-form adjoint the header comment of mp_tr_composite_geometry_bwd gives."""
import numpy as np
import torch

from tests import geometry_reference as G

DIFF_KEYS = ("depth", "depth_person", "acc_solo", "depth_solo", "depth_solo_level")

# the ragged cases of the C-ABI tests: ((R, P, n_z), beta, level)
CASES = [((70, 3, 98), 0.1, 0.5),     # RAGGED_HITS: rays hit by 0 / 1 / 2 / 3 persons; S = 97: two 64-lane passes
         ((70, 3, 98), 0.02, 0.5),
         ((70, 3, 98), 0.1, 0.9),
         ((5, 1, 65), 0.001, 0.5),    # S = 64: exactly one pass
         ((9, 2, 34), 0.02, 0.5),
         ((13, 8, 130), 0.1, 0.5)]    # the person limit, three passes


def case_hits(R, P):
    """ray 0 hit by nobody, ray 1 by person 0 alone, the rest by all persons or by a ragged subset"""
    if (R, P) == (70, 3):
        return G.RAGGED_HITS
    return [np.arange(1, R)] + [np.array([r for r in range(2, R) if (r + n) % 5 != 0]) for n in range(1, P)]


def case(shape, beta, level, seed=4):
    """-> inv, z, sdf (float32 numpy, G.ragged_case), the float64 forward reference, and seeded normal upstream gradients with the
    level term zeroed on the (ray, person) entries a float32 implementation may cross one sample off (G.exempt)"""
    R, P, NZ = shape
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=seed, hits=case_hits(R, P))
    ref = G.geometry_reference(R, inv, z, sdf, beta, level)
    rs = np.random.RandomState(100 + seed)
    up = dict(depth=rs.randn(R), depth_person=rs.randn(R, P), acc_solo=rs.randn(R, P), depth_solo=rs.randn(R, P),
              depth_solo_level=rs.randn(R, P))
    up = {k: v.astype(np.float32) for k, v in up.items()}
    up["depth_solo_level"][G.exempt(ref["fe_cross_solo"], ref["margin_solo"])] = 0.0
    return inv, z, sdf, ref, up


def laplace_density(sdf, beta):
    """density.py:20-29: (1/beta) (0.5 + 0.5 sign(s) expm1(-|s|/beta))"""
    return (1.0 / beta) * (0.5 + 0.5 * torch.sign(sdf) * torch.expm1(-sdf.abs() / beta))


def _sorted_list(ts, te, fe, who):
    """samples in the order of the key (t_end, person); stable, so a person's own samples keep their order"""
    order = sorted(range(len(te)), key=lambda j: (float(te[j].detach()), int(who[j])))
    idx = torch.tensor(order, dtype=torch.long)
    return ts[idx], te[idx], fe[idx], who[idx]


def _sums(ts, te, fe):
    E = torch.cumsum(fe, 0) - fe                                     # free energy in front of every sample
    w = (1.0 - torch.exp(-fe)) * torch.exp(-E)
    return E, w, 0.5 * (ts + te)


def geometry_outputs(n_rays, inv_index, z, sdf, beta, level=0.5):
    """inv_index[n] (R,) ints, z[n] (R_n, S+1) and sdf[n] (R_n, S) torch tensors (sdf may require grad), beta a 0-d tensor (may
    require grad).  -> {depth (R,), depth_person, acc_solo, depth_solo, depth_solo_level (R,P)} with autograd history."""
    P, R = len(inv_index), int(n_rays)
    L = G.level_energy(level)
    dt = z[0].dtype
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    zero, minus = torch.zeros((), dtype=dt), -torch.ones((), dtype=dt)
    rows = {k: [] for k in DIFF_KEYS}
    for r in range(R):
        parts, cols = [], {k: [zero] * P for k in DIFF_KEYS[1:]}
        cols["depth_solo_level"] = [minus] * P
        for n in range(P):
            k = int(inv[n][r])
            if k < 0:
                continue
            ts, te = z[n][k, :-1], z[n][k, 1:]
            fe = laplace_density(sdf[n][k], beta) * (te - ts)
            who = torch.full((len(te),), n, dtype=torch.long)
            parts.append((ts, te, fe, who))
            s_ts, s_te, s_fe, _ = _sorted_list(ts, te, fe, who)      # person n alone
            E, w, tm = _sums(s_ts, s_te, s_fe)
            cols["acc_solo"][n], cols["depth_solo"][n] = w.sum(), (w * tm).sum()
            hit = torch.nonzero((E + s_fe).detach() >= L).flatten()
            if len(hit):
                j = int(hit[0])
                f = torch.clamp((L - E[j]) / s_fe[j], 0.0, 1.0) if float(s_fe[j].detach()) > 0 else zero
                cols["depth_solo_level"][n] = s_ts[j] + (s_te[j] - s_ts[j]) * f
        depth = zero
        if parts:
            ts, te, fe, who = _sorted_list(*[torch.cat([q[a] for q in parts]) for a in range(4)])
            E, w, tm = _sums(ts, te, fe)
            depth = (w * tm).sum()
            for n in range(P):
                cols["depth_person"][n] = ((w * tm)[who == n]).sum()
        rows["depth"].append(depth)
        for k in DIFF_KEYS[1:]:
            rows[k].append(torch.stack(cols[k]))
    return {k: torch.stack(v) for k, v in rows.items()}


def adjoint_formulas(n_rays, inv_index, z, sdf, beta, level, up):
    """float64 numpy evaluation of the closed-form adjoint.  up: {key of DIFF_KEYS: upstream gradient or None}.
    -> (d_sdf list of (R_n, S), d_beta)"""
    P, R = len(inv_index), int(n_rays)
    L = G.level_energy(level)
    beta = float(beta)
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    z = [np.asarray(a, dtype=np.float64) for a in z]
    sdf = [np.asarray(a, dtype=np.float64) for a in sdf]
    g = {k: (None if up.get(k) is None else np.asarray(up[k], dtype=np.float64)) for k in DIFF_KEYS}
    at = lambda k, *i: 0.0 if g[k] is None else float(g[k][i])
    d_sdf = [np.zeros_like(s) for s in sdf]
    d_beta = 0.0
    for r in range(R):
        ps = [n for n in range(P) if inv[n][r] >= 0]
        if not ps:
            continue
        ts = {n: z[n][inv[n][r], :-1] for n in ps}
        te = {n: z[n][inv[n][r], 1:] for n in ps}
        fe = {n: G.laplace_density(sdf[n][inv[n][r]], beta) * (te[n] - ts[n]) for n in ps}
        dfe = {n: np.zeros_like(fe[n]) for n in ps}
        # merged sums
        key = sorted((te[n][i], n, i) for n in ps for i in range(len(te[n])))
        m_n, m_i = np.array([a[1] for a in key]), np.array([a[2] for a in key])
        m_fe = np.array([fe[n][i] for _, n, i in key])
        m_tm = np.array([0.5 * (ts[n][i] + te[n][i]) for _, n, i in key])
        E = np.cumsum(m_fe) - m_fe
        w = (1 - np.exp(-m_fe)) * np.exp(-E)
        dw = np.array([at("depth", r) + at("depth_person", r, n) for n in m_n]) * m_tm
        behind = np.cumsum((dw * w)[::-1])[::-1] - dw * w
        m_dfe = dw * np.exp(-E) * np.exp(-m_fe) - behind
        for a, (n, i) in enumerate(zip(m_n, m_i)):
            dfe[n][i] += m_dfe[a]
        for n in ps:
            # solo sums
            tm = 0.5 * (ts[n] + te[n])
            Es = np.cumsum(fe[n]) - fe[n]
            w0 = (1 - np.exp(-fe[n])) * np.exp(-Es)
            dws = at("acc_solo", r, n) + at("depth_solo", r, n) * tm
            dfe[n] += dws * np.exp(-Es) * np.exp(-fe[n]) - (np.cumsum((dws * w0)[::-1])[::-1] - dws * w0)
            # solo level depth
            hit = np.nonzero(Es + fe[n] >= L)[0]
            if len(hit) and fe[n][hit[0]] > 0:
                j = hit[0]
                f = (L - Es[j]) / fe[n][j]
                if 0 < f < 1:
                    c = at("depth_solo_level", r, n) * (te[n][j] - ts[n][j]) / fe[n][j]
                    dfe[n][:j] -= c
                    dfe[n][j] -= c * f
            # d fe -> d sigma -> d sdf, d beta
            s = sdf[n][inv[n][r]]
            dsig = dfe[n] * (te[n] - ts[n])
            eab = np.exp(-np.abs(s) / beta)
            dbe = np.where(s > 0, 0.5 / beta**2 * eab * (s / beta - 1),
                           np.where(s < 0, -1 / beta**2 + 0.5 / beta**2 * eab * (1 + s / beta), -0.5 / beta**2))
            d_sdf[n][inv[n][r]] += dsig * (-(0.5 / beta**2) * eab)
            d_beta += float((dsig * dbe).sum())
    return d_sdf, d_beta


def autograd_gradients(n_rays, inv_index, z, sdf, beta, level, up):
    """float64 autograd of sum_k <up[k], geometry_outputs[k]> -> (d_sdf list of (R_n, S) numpy, d_beta float)"""
    zt = [torch.tensor(np.asarray(a), dtype=torch.float64) for a in z]
    st = [torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True) for a in sdf]
    bt = torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    out = geometry_outputs(n_rays, inv_index, zt, st, bt, level)
    loss = bt * 0.0 + sum(s.sum() * 0.0 for s in st)
    for k in DIFF_KEYS:
        if up.get(k) is not None:
            loss = loss + (torch.tensor(np.asarray(up[k]), dtype=torch.float64) * out[k]).sum()
    loss.backward()
    return [s.grad.numpy() for s in st], float(bt.grad)
