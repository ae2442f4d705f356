"""Float64 reference of mp_composite_geometry (include/multiply_hip.h), written from the definitions and not from the kernel:
a plain loop over the rays that builds each ray's merged sample list by actually sorting the key (t_end, person), then takes
cumulative sums along that list.  No rank lookups, no per-person prefix sums.

Alongside the seven outputs it returns, per ray (merged) and per ray and person (solo), what the tests need to bound a float32
implementation: the crossing sample's free energy and interval, the intervals of its neighbours in merged order, and the
smallest |E + fe - L| over the ray's samples (a ray on which that margin is tiny may legitimately cross one sample earlier or
later in float32)."""
import math

import numpy as np


def laplace_density(sdf, beta):
    """density.py:20-29 in float64: (1/beta) (0.5 + 0.5 sign(s) expm1(-|s|/beta))"""
    return (1.0 / beta) * (0.5 + 0.5 * np.sign(sdf) * np.expm1(-np.abs(sdf) / beta))


def level_energy(level):
    """L = -ln(1 - level) of the float32 level the C ABI receives"""
    return -math.log1p(-float(np.float32(level)))


def _one_list(ts, te, fe, who, L, P):
    """One ray's samples (any order) -> sums and the level crossing.  `who` = the person column of every sample."""
    n = len(te)
    out = dict(acc=0.0, depth=0.0, acc_person=np.zeros(P), depth_person=np.zeros(P), level=-1.0, front=-1,
               fe_cross=np.inf, margin=np.inf, slope=0.0, near=np.zeros((0, 2)), near_last=True, total=0.0)
    if n == 0:
        return out
    order = sorted(range(n), key=lambda j: (te[j], who[j]))          # stable: a person's own samples keep their order
    ts, te, fe, who = ts[order], te[order], fe[order], who[order]
    E = np.concatenate([[0.0], np.cumsum(fe)[:-1]])                  # free energy in front of every sample
    w = (1.0 - np.exp(-fe)) * np.exp(-E)
    tm = 0.5 * (ts + te)
    out["acc"], out["depth"], out["total"] = w.sum(), (w * tm).sum(), fe.sum()
    for p in range(P):
        out["acc_person"][p] = w[who == p].sum()
        out["depth_person"][p] = (w * tm)[who == p].sum()
    out["margin"] = np.abs(E + fe - L).min()
    hit = np.nonzero(E + fe >= L)[0]
    if len(hit):
        j = hit[0]                                                   # = the minimum of (te, person) over the satisfying samples
        f = min(max((L - E[j]) / fe[j], 0.0), 1.0) if fe[j] > 0 else 0.0
        out["level"] = ts[j] + (te[j] - ts[j]) * f
        out["front"] = int(who[j])
        out["fe_cross"] = fe[j]
        out["slope"] = (te[j] - ts[j]) / fe[j] if fe[j] > 0 else np.inf
        lo, hi = max(j - 1, 0), min(j + 1, n - 1)
        out["near"] = np.stack([ts[lo:hi + 1], te[lo:hi + 1]], 1)
        out["near_last"] = bool(hi == n - 1)
    else:                                                            # no crossing: the nearest miss is past the last sample
        out["near"] = np.stack([ts[-1:], te[-1:]], 1)
    return out


def geometry_reference(n_rays, inv_index, z, sdf, beta, level=0.5):
    """inv_index[n] (R,) int, z[n] (R_n, S+1), sdf[n] (R_n, S) for the P composited persons, in column order.
    -> dict: depth (R,), depth_person (R,P), depth_level (R,), front_person (R,), acc_solo / depth_solo / depth_solo_level (R,P),
    plus acc (R,), acc_person (R,P) (the weight sums, = mp_composite's acc_map / acc_person) and the diagnostics
    fe_cross / margin / slope / total (R,) and *_solo (R,P), near (per ray the (k,2) intervals [ts, te] of the crossing sample and
    its neighbours in merged order; of the last sample where nothing crosses), near_last (the last sample is among them: an
    implementation one sample late finds no crossing) and near_solo[r][n] / near_last_solo."""
    P = len(inv_index)
    R = int(n_rays)
    beta = float(np.float32(beta))
    L = level_energy(level)
    inv = [np.asarray(a).astype(np.int64).reshape(-1) for a in inv_index]
    z = [np.asarray(a, dtype=np.float64) for a in z]
    sdf = [np.asarray(a, dtype=np.float64) for a in sdf]
    o = dict(depth=np.zeros(R), depth_person=np.zeros((R, P)), depth_level=np.full(R, -1.0), front_person=np.full(R, -1, np.int64),
             acc_solo=np.zeros((R, P)), depth_solo=np.zeros((R, P)), depth_solo_level=np.full((R, P), -1.0),
             acc=np.zeros(R), acc_person=np.zeros((R, P)), fe_cross=np.full(R, np.inf), margin=np.full(R, np.inf),
             slope=np.zeros(R), total=np.zeros(R), fe_cross_solo=np.full((R, P), np.inf), margin_solo=np.full((R, P), np.inf),
             slope_solo=np.zeros((R, P)), total_solo=np.zeros((R, P)), near=[None] * R, near_solo=[[None] * P for _ in range(R)],
             near_last=np.ones(R, bool), near_last_solo=np.ones((R, P), bool), L=L)
    for r in range(R):
        parts = []
        for n in range(P):
            k = inv[n][r]
            if k < 0:
                o["near_solo"][r][n] = np.zeros((0, 2))
                continue
            ts, te = z[n][k, :-1], z[n][k, 1:]
            fe = laplace_density(sdf[n][k], beta) * (te - ts)
            who = np.full(len(te), n)
            parts.append((ts, te, fe, who))
            s = _one_list(ts, te, fe, who, L, P)                     # person n alone
            o["acc_solo"][r, n], o["depth_solo"][r, n], o["depth_solo_level"][r, n] = s["acc"], s["depth"], s["level"]
            o["fe_cross_solo"][r, n], o["margin_solo"][r, n], o["slope_solo"][r, n] = s["fe_cross"], s["margin"], s["slope"]
            o["total_solo"][r, n] = s["total"]
            o["near_solo"][r][n], o["near_last_solo"][r, n] = s["near"], s["near_last"]
        if parts:
            m = _one_list(*[np.concatenate([q[a] for q in parts]) for a in range(4)], L, P)
        else:
            m = _one_list(*[np.zeros(0)] * 4, L, P)
        o["depth"][r], o["depth_person"][r], o["depth_level"][r], o["front_person"][r] = m["depth"], m["depth_person"], m["level"], m["front"]
        o["acc"][r], o["acc_person"][r] = m["acc"], m["acc_person"]
        o["fe_cross"][r], o["margin"][r], o["slope"][r], o["total"][r], o["near"][r] = m["fe_cross"], m["margin"], m["slope"], m["total"], m["near"]
        o["near_last"][r] = m["near_last"]
    return o


def exempt(fe_cross, margin):
    """A crossing a float32 implementation may place one sample off: the crossing sample is almost empty (fe < 1e-3) or some
    sample's E + fe lies within 1e-4 of L."""
    return (np.asarray(fe_cross) < 1e-3) | (np.asarray(margin) < 1e-4)


def ragged_case(R, P, n_z, seed=4, hits=None):
    """Seeded inputs in the style of test_composite_backward (float32 numpy): sorted depths in [1, 3], sdf ~ N(0, 0.05).
    hits[n] = the ascending rays person n is hit on (default: all rays for every person).
    -> inv_index (P x (R,) int32), z (P x (R_n, n_z)), sdf (P x (R_n, n_z - 1))"""
    rs = np.random.RandomState(seed)
    if hits is None:
        hits = [np.arange(R)] * P
    inv, z, sdf = [], [], []
    for n in range(P):
        h = np.asarray(hits[n])
        iv = np.full(R, -1, np.int32)
        iv[h] = np.arange(len(h), dtype=np.int32)
        inv.append(iv)
        rows = max(len(h), 1)
        z.append(np.sort(rs.rand(rows, n_z).astype(np.float32) * 2.0 + 1.0, axis=1))
        sdf.append((rs.randn(rows, n_z - 1) * 0.05).astype(np.float32))
    return inv, z, sdf


# the hit sets of test_composite_backward plus a third person: rays hit by none (65..69), one, two and all three persons
RAGGED_HITS = [np.arange(0, 50), np.arange(30, 65), np.arange(10, 40)]
