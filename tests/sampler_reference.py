"""The error-bound sampler stage by stage, in plain torch (reference ray_sampler.py:66-230 as oracle/multiply_oracle.py:348-479
restates it), plus the seeded input states of tests/test_sampler_kernels_gpu.py.

Every stage works in the dtype of the tensors it is handed: float64 is the reference, float32 the host's own evaluation of
the same formulas (the CPU spreads of tests/tolerances_sampler.py and the set of `sharp` rays come from comparing the two;
nothing here ever sees device output).  The residual checks of the GPU file do not predict the kernels' results with these
functions: they evaluate them AT the kernels' results (error_bound at the returned beta, cdf_interval at the returned depth).
"""
import math

import numpy as np
import torch

F64 = torch.float64


# ================================================================================================ stages
def beta_init(z, eps):
    """the upper bound's beta of ray_sampler.py:74-76 on the depths z (R, NE)"""
    d = z[:, 1:] - z[:, :-1]
    return torch.sqrt((1.0 / (4.0 * math.log(eps + 1.0))) * (d ** 2.0).sum(-1))


def init_depths(near, far, NE, t_rand=None, eps=0.1):
    """UniformSampler.get_z_vals (ray_sampler.py:21-42) + the first beta -> znew (R, NE), beta_init (R,).  far (R,)."""
    dt = far.dtype
    t = torch.linspace(0.0, 1.0, NE, dtype=dt)
    z = near * (1.0 - t) + far[:, None] * t
    if t_rand is not None:
        mids = 0.5 * (z[:, 1:] + z[:, :-1])
        upper = torch.cat([mids, z[:, -1:]], -1)
        lower = torch.cat([z[:, :1], mids], -1)
        z = lower + (upper - lower) * t_rand.to(dt)
    return z, beta_init(z, eps)


def merge(z_old, s_old, z_new, s_new):
    """sort of cat([old, new]) (ray_sampler.py:89-94, 191) as a STABLE merge: on equal depth the old entries come first"""
    z = torch.cat([z_old, z_new], -1)
    s = torch.cat([s_old, s_new], -1)
    Z, idx = torch.sort(z, dim=-1, stable=True)
    return Z, torch.gather(s, 1, idx)


def d_star_branches(Z, S):
    """(first, second, heron) masks (R, n-1) of Theorem 1's three cases (ray_sampler.py:98-107); `second` wins over `first`
    where both hold, as the reference's successive masked assignments do"""
    a, b, c = Z[:, 1:] - Z[:, :-1], S[:, :-1].abs(), S[:, 1:].abs()
    first = a.pow(2) + b.pow(2) <= c.pow(2)
    second = a.pow(2) + c.pow(2) <= b.pow(2)
    heron = ~first & ~second & (b + c - a > 0)
    return first & ~second, second, heron


def d_star(Z, S):
    """ray_sampler.py:98-110: the three branches and the sign product -> (R, n-1)"""
    a, b, c = Z[:, 1:] - Z[:, :-1], S[:, :-1].abs(), S[:, 1:].abs()
    first, second, heron = d_star_branches(Z, S)
    s = (a + b + c) / 2.0
    area = s * (s - a) * (s - b) * (s - c)
    d = torch.zeros_like(a)
    d = torch.where(first, b, d)
    d = torch.where(second, c, d)
    d = torch.where(heron, (2.0 * torch.sqrt(area)) / torch.where(heron, a, torch.ones_like(a)), d)
    same = (S[:, 1:].sign() * S[:, :-1].sign()) == 1
    return torch.where(same, d, torch.zeros_like(d))


def density(S, beta):
    """LaplaceDensity (density.py:20-29)"""
    return (1.0 / beta) * (0.5 + 0.5 * S.sign() * torch.expm1(-S.abs() / beta))


def _col(beta, like):
    beta = torch.as_tensor(beta, dtype=like.dtype)
    return beta.reshape(-1, 1) if beta.dim() else beta


def error_bound(Z, S, beta, dstar=None):
    """get_error_bound (ray_sampler.py:222-230): one scalar per ray; beta a scalar or (R,).  A NaN sdf gives NaN."""
    beta = _col(beta, Z)
    dists = Z[:, 1:] - Z[:, :-1]
    d = d_star(Z, S) if dstar is None else dstar
    dens = density(S, beta)
    shifted = torch.cat([torch.zeros_like(Z[:, :1]), dists * dens[:, :-1]], -1)
    integral = torch.cumsum(shifted, -1)
    err_sec = torch.exp(-d / beta) * (dists ** 2.0) / (4 * beta ** 2)
    err_int = torch.cumsum(err_sec, -1)
    bound = (torch.clamp(torch.exp(err_int), max=1.0e6) - 1.0) * torch.exp(-integral[:, :-1])
    return bound.max(-1)[0]


def line_search(Z, S, beta_prev, beta0, eps, iters):
    """ray_sampler.py:113-122 -> beta (R,)"""
    d = d_star(Z, S)
    beta = beta_prev.clone()
    curr = error_bound(Z, S, beta0, d)
    beta[curr <= eps] = beta0
    bmin, bmax = beta0 * torch.ones_like(beta), beta
    for _ in range(iters):
        mid = (bmin + bmax) / 2.0
        ok = error_bound(Z, S, mid, d) <= eps
        bmax = torch.where(ok, mid, bmax)
        bmin = torch.where(~ok, mid, bmin)
    return bmax


def pdf_cdf(Z, S, beta, more, add_tiny):
    """ray_sampler.py:126-166 -> cdf (R, n): `more`: the error-bound pdf + add_tiny, else the weights + 1e-5 (whose last
    distance is 1e10)"""
    beta = _col(beta, Z)
    R = Z.shape[0]
    dists = Z[:, 1:] - Z[:, :-1]
    dens = density(S, beta)
    dists_inf = torch.cat([dists, 1e10 * torch.ones(R, 1, dtype=Z.dtype)], -1)
    free = dists_inf * dens
    shifted = torch.cat([torch.zeros(R, 1, dtype=Z.dtype), free[:, :-1]], -1)
    alpha = 1 - torch.exp(-free)
    trans = torch.exp(-torch.cumsum(shifted, -1))
    if more:
        err_sec = torch.exp(-d_star(Z, S) / beta) * (dists ** 2.0) / (4 * beta ** 2)
        err_int = torch.cumsum(err_sec, -1)
        pdf = (torch.clamp(torch.exp(err_int), max=1.0e6) - 1.0) * trans[:, :-1] + add_tiny
    else:
        pdf = (alpha * trans)[:, :-1] + 1e-5
    pdf = pdf / pdf.sum(-1, keepdim=True)
    return torch.cat([torch.zeros(R, 1, dtype=Z.dtype), torch.cumsum(pdf, -1)], -1)


def inverse_cdf(Z, cdf, u):
    """ray_sampler.py:174-186"""
    inds = torch.searchsorted(cdf, u, right=True)
    below = torch.clamp(inds - 1, min=0)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    zb, za = torch.gather(Z, 1, below), torch.gather(Z, 1, above)
    denom = ca - cb
    denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return zb + (u - cb) / denom * (za - zb)


def extra_indices(n, NX):
    """the eval picks of ray_sampler.py:204: torch's own linspace and truncation, in torch's default dtype like the reference"""
    return torch.linspace(0, n - 1, NX).long()


def cdf_interval(Z, cdf, z):
    """F(z) of ONE ray as [F_lo, F_hi] plus the local slope.  F is the piecewise-linear function through (Z_i, cdf_i); where
    depths repeat F jumps and the interval is the whole jump, elsewhere F_lo == F_hi.  Z, cdf (n,), z (m,), numpy float64;
    z must lie in [Z[0], Z[n-1]].  slope: the largest slope of F over the bins that touch z (0 at a pure jump)."""
    Z, cdf, z = np.asarray(Z, np.float64), np.asarray(cdf, np.float64), np.asarray(z, np.float64)
    n = Z.shape[0]
    lo = np.searchsorted(Z, z, side="left")       # first index with Z >= z
    hi = np.searchsorted(Z, z, side="right")      # first index with Z > z
    assert (lo < n).all() and (hi > 0).all(), "depth outside the list"
    at_knot = hi > lo
    F_lo, F_hi, slope = np.empty_like(z), np.empty_like(z), np.zeros_like(z)
    F_lo[at_knot], F_hi[at_knot] = cdf[lo[at_knot]], cdf[hi[at_knot] - 1]

    def bin_slope(i):       # bin [i, i+1], i clipped into range; empty bins (a jump) have none
        i = np.clip(i, 0, n - 2)
        w = Z[i + 1] - Z[i]
        return np.where(w > 0, (cdf[i + 1] - cdf[i]) / np.where(w > 0, w, 1.0), 0.0)

    slope[at_knot] = np.maximum(bin_slope(lo[at_knot] - 1), bin_slope(hi[at_knot] - 1))
    inn = ~at_knot
    i = lo[inn] - 1
    t = (z[inn] - Z[i]) / (Z[i + 1] - Z[i])
    F_lo[inn] = F_hi[inn] = cdf[i] + t * (cdf[i + 1] - cdf[i])
    slope[inn] = bin_slope(i)
    return F_lo, F_hi, slope


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


# ================================================================================================ the whole chain
def run_chain(cfg, near, far, sdf_of_z, beta0, draws=None):
    """ErrorBoundSampler.get_z_vals chained from the stages above, one convergence vote over all rays ->
    (z_out (R, N + N_extra + 2), iterations).  cfg: an oracle SamplerCfg; sdf_of_z(z (R, m)) -> sdf (R, m)."""
    NE, R = cfg.N_samples_eval, far.shape[0]
    z_new, beta = init_depths(near, far, NE, None if draws is None else draws["t_rand"], cfg.eps)
    Z, S = z_new[:, :0], z_new[:, :0]
    it = 0
    while True:
        Z, S = merge(Z, S, z_new, sdf_of_z(z_new))
        beta = line_search(Z, S, beta, beta0, cfg.eps, cfg.beta_iters)
        it += 1
        more = bool(beta.max() > beta0) and it < cfg.max_total_iters
        cdf = pdf_cdf(Z, S, beta, more, cfg.add_tiny)
        N = NE if more else cfg.N_samples
        if more or draws is None:
            u = torch.linspace(0.0, 1.0, N, dtype=Z.dtype)[None].repeat(R, 1)
        else:
            u = draws["u_final"].to(Z.dtype)
        samples = inverse_cdf(Z, cdf, u.contiguous())
        if not more:
            break
        z_new = samples
    n = Z.shape[1]
    parts = [samples, near * torch.ones(R, 1, dtype=Z.dtype), far[:, None]]
    if cfg.N_samples_extra > 0:
        idx = extra_indices(n, cfg.N_samples_extra) if draws is None else draws["extra_idx"][n // NE - 1].long()
        parts.append(Z[:, idx])
    return torch.sort(torch.cat(parts, -1), -1)[0], it


# ================================================================================================ the scene of the inputs
CAM_DIST, SPHERE_R, BOUND_R = 3.0, 0.6, 3.0
MAX_RAYS, N_TOTAL, GROUP = 37, 40, 8
N_GROUPS = (N_TOTAL + GROUP - 1) // GROUP
NOT_HIT = (5, 17, 30)                       # the rays of the call that are not in hit_index
INACTIVE = (4, 20)                          # hit rays whose ray_active is 0 in the bound / resample states
NAN_RAY = 11                                # the hit ray that carries a NaN in sdfnew (bound states)
NEAR = 0.0


def hit_index():
    return np.array([r for r in range(N_TOTAL) if r not in NOT_HIT], dtype=np.int32)


def impacts():
    """impact parameters of the 37 hit rays: 28 through the sphere (<= 0.5), 9 grazing or missing it (0.58 .. 0.9), mixed
    over the convergence groups by a fixed permutation"""
    b = np.concatenate([np.linspace(0.0, 0.5, 28), np.linspace(0.58, 0.9, 9)])
    return b[np.random.default_rng(7).permutation(MAX_RAYS)]


def ray_far(b):
    """far root of the ray with impact parameter b on the bounding sphere the camera sits on"""
    return 2.0 * CAM_DIST * np.sqrt(1.0 - (b / CAM_DIST) ** 2)


def sphere_sdf(z, b):
    """signed distance to the sphere at depth z of the ray with impact parameter b (z (R, m), b (R,)), float64"""
    cos = np.sqrt(1.0 - (b / CAM_DIST) ** 2)[:, None]
    return np.sqrt(np.maximum(z * z - 2.0 * CAM_DIST * cos * z + CAM_DIST ** 2, 0.0)) - SPHERE_R


def far_table():
    """far of all 40 rays of the call (float32); the rays outside hit_index carry a value no hit ray has"""
    far = np.full(N_TOTAL, 99.0, np.float32)
    far[hit_index()] = ray_far(impacts()).astype(np.float32)
    return far


def _focus(b):
    """where a ray's samples concentrate: the surface entry, or the closest approach of a ray that misses"""
    cos = np.sqrt(1.0 - (b / CAM_DIST) ** 2)
    return CAM_DIST * cos - np.sqrt(np.maximum(SPHERE_R ** 2 - b ** 2, 0.0))


def _sdf_family(g, z, b, family):
    """sdf values (float32) at the float32 depths z: every entry carries its own 1e-4 noise, so that entries of equal depth
    are told apart and a wrong tie order shows"""
    z64 = z.astype(np.float64)
    k = np.arange(z.shape[0])[:, None]
    if family == "random":
        s = g.uniform(-0.3, 0.8, z.shape)
    else:
        s = sphere_sdf(z64, b) + 1e-4 * g.standard_normal(z.shape)
        if family == "perturbed":
            s = s + 0.03 * np.sin(25.0 * z64 + k)
    return s.astype(np.float32)


def _chunk(g, NE, b, far, sigma):
    """NE depths per ray around the ray's focus, clipped to [near, far]; from NE = 4 on two of them are near and far themselves
    (what the inverse CDF returns at u = 0 and u = 1), with NE = 2 one is"""
    R = b.shape[0]
    z = _focus(b)[:, None] + sigma[:, None] * g.standard_normal((R, NE))
    z = np.clip(z, NEAR, far[:, None].astype(np.float64)).astype(np.float32)
    if NE >= 4:
        z[:, 0], z[:, 1] = NEAR, far
    else:
        odd = (np.arange(R) % 2).astype(bool)
        z[odd, 0], z[~odd, 1] = NEAR, far[~odd]
    return np.sort(z, -1)


def bound_case(NE, n_old, beta0, family, seed):
    """One state of k_sampler_bound for the 37 hit rays: z_old / s_old (R, n_old) sorted, z_new / s_new (R, NE) sorted, beta_prev
    (R,), all float32.  Ties on purpose: z_new holds near, far and copies of z_old entries, both lists hold a repeated depth.
    Ray NAN_RAY has a NaN in s_new.  beta_prev - beta0 >= 0.1 beta0 on every ray."""
    g = np.random.default_rng(seed)
    b = impacts()
    far = ray_far(b).astype(np.float32)
    R = MAX_RAYS
    sigma = 10.0 ** g.uniform(-2.5, -0.5, R)
    uniform = np.stack([np.linspace(NEAR, f, NE) for f in far.astype(np.float64)]).astype(np.float32)
    if n_old:
        chunks = [uniform] + [_chunk(g, NE, b, far, sigma) for _ in range(n_old // NE - 1)]
        z_old = np.sort(np.concatenate(chunks, -1), -1)
        if n_old >= 4:
            z_old[:, n_old // 2] = z_old[:, n_old // 2 - 1]                  # a repeated depth inside zs
        z_new = _chunk(g, NE, b, far, sigma)
        for j in range(min(3, NE // 4)):                                     # depths of zs repeated in znew
            z_new[:, 2 + j] = z_old[np.arange(R), g.integers(0, n_old, R)]
        z_new = np.sort(z_new, -1)
    else:
        z_old = np.zeros((R, 0), np.float32)
        z_new = uniform.copy()
    if NE >= 4:
        z_new[:, NE // 2] = z_new[:, NE // 2 - 1]                            # a repeated depth inside znew
    s_old, s_new = _sdf_family(g, z_old, b, family), _sdf_family(g, z_new, b, family)
    s_new[NAN_RAY, NE // 2] = np.nan
    if n_old:
        beta_prev = np.float32(beta0) * (1.1 + 10.0 ** g.uniform(-1.0, 1.3, R)).astype(np.float32)
    else:                                                                    # the first iteration starts from the upper bound
        beta_prev = beta_init(torch.from_numpy(z_new).to(F64), float(np.float32(0.1))).numpy().astype(np.float32)
        beta_prev = np.maximum(beta_prev, np.float32(1.2 * beta0))
    return dict(NE=NE, n_old=n_old, beta0=np.float32(beta0), z_old=z_old, s_old=s_old, z_new=z_new, s_new=s_new,
                beta_prev=beta_prev.astype(np.float32), far=far, b=b)


RESAMPLE_BETAS = (0.1, 0.03, 0.01, 0.003, 0.001)


def resample_case(NE, n, seed, family="sphere", inverted=False):
    """One state of k_sampler_resample: Z / S (R, n) float32 with DISTINCT ascending depths per ray, Z[0] = near, Z[n-1] = far,
    and beta (R,) cycling through RESAMPLE_BETAS.  inverted: rays with an odd index carry one adjacent pair of depths swapped
    by one float32 step in the middle of the list (the state of the fallback-sort case)."""
    g = np.random.default_rng(seed)
    b = impacts()
    far = ray_far(b).astype(np.float32)
    R = MAX_RAYS
    sigma = 10.0 ** g.uniform(-2.0, -0.5, R)
    Z = np.empty((R, n), np.float32)
    for k in range(R):
        cand = np.concatenate([np.linspace(NEAR, float(far[k]), n + 2)[1:-1],
                               _focus(b[k:k + 1])[0] + sigma[k] * g.standard_normal(2 * n)]).astype(np.float32)
        cand = np.unique(cand[(cand > NEAR) & (cand < far[k])])
        Z[k] = np.concatenate([[np.float32(NEAR)], np.sort(g.choice(cand, n - 2, replace=False)), [far[k]]])
    S = _sdf_family(g, Z, b, family)
    if inverted:
        m = n // 2
        for k in range(1, R, 2):
            S[k] = 2.0                                              # far from any surface: every bin weighs the same
            Z[k, m + 1] = np.nextafter(Z[k, m], np.float32(-np.inf))
            assert Z[k, m - 1] < Z[k, m + 1] < Z[k, m] < Z[k, m + 2]
    beta = np.array([RESAMPLE_BETAS[k % len(RESAMPLE_BETAS)] for k in range(R)], np.float32)
    return dict(NE=NE, n=n, Z=Z, S=S, beta=beta, far=far, b=b)


def cdfs(case, more, add_tiny, dtype=F64):
    """cdf (R, n) of a resample state in `dtype`, from the state's float32 values"""
    return pdf_cdf(torch.from_numpy(case["Z"]).to(dtype), torch.from_numpy(case["S"]).to(dtype),
                   torch.from_numpy(case["beta"]).to(dtype), more, float(np.float32(add_tiny)))


SHARP_LIMIT = 1e-5


def cdf_spread(case, more, add_tiny):
    """per ray, max |cdf32 - cdf64| of the reference's own two evaluations"""
    return (cdfs(case, more, add_tiny, torch.float32).to(F64) - cdfs(case, more, add_tiny)).abs().amax(-1).numpy()


def sharp_rays(case, more, add_tiny):
    """the rays whose reference cdf agrees between float32 and float64 to SHARP_LIMIT: the rays whose samples are value-checked"""
    return cdf_spread(case, more, add_tiny) <= SHARP_LIMIT


# the cases of the GPU file (shared with the CPU file, which asserts the input conditions on them)
EPS, ADD_TINY = 0.1, 1e-6
LINE_SEARCH_CASES = [            # (NE, n_old, beta0, family, max_total_iters)
    (64, 0, 0.1, "sphere", 5), (64, 64, 0.01, "perturbed", 5), (65, 195, 0.001, "sphere", 5),
    (128, 384, 0.01, "sphere", 5), (128, 128, 0.1, "random", 5), (64, 192, 0.001, "perturbed", 5),
    (65, 65, 0.1, "perturbed", 5), (128, 256, 0.001, "sphere", 5),
]
LARGE_BOUND_CASES = [(128, 640, 0.01, "sphere", 8), (128, 896, 0.001, "perturbed", 8)]
RESAMPLE_CASES = [               # (NE, n, max_total_iters, iter, family)
    (64, 64, 5, 0, "sphere"), (64, 320, 5, 4, "sphere"), (64, 192, 5, 2, "perturbed"),
]
LARGE_RESAMPLE_CASES = [(128, 768, 8, 5, "sphere"), (128, 1024, 8, 7, "sphere")]
INVERTED_NE, INVERTED_NS, INVERTED_NX = 8, 24, 8      # the fallback-sort case: few wide bins, several samples in each


def case_seed(*key):
    """a seed that depends on the case alone (not on the process: no hash())"""
    import zlib
    return zlib.crc32(repr(tuple(key)).encode())


def merged(case):
    """float64 (Z, S) of a bound state after the stable merge"""
    t = {k: torch.from_numpy(case[k]).to(F64) for k in ("z_old", "s_old", "z_new", "s_new")}
    return merge(t["z_old"], t["s_old"], t["z_new"], t["s_new"])


def root_spread(case, eps=EPS):
    """On the rays whose float64 error bound crosses eps between beta0 and beta_prev: the float64 root of E(beta) = eps by
    bisection and |E32(root) - E64(root)| / E64(root) -> (spreads, log-slopes |d ln E / d ln beta| at the root)"""
    Z, S = merged(case)
    ok = ~torch.isnan(S).any(-1)
    Z, S = Z[ok], S[ok]
    eps64 = float(np.float32(eps))
    b0 = torch.full((Z.shape[0],), float(case["beta0"]), dtype=F64)
    b1 = torch.from_numpy(case["beta_prev"]).to(F64)[ok]
    d = d_star(Z, S)
    cross = (error_bound(Z, S, b0, d) > eps64) & (error_bound(Z, S, b1, d) <= eps64)
    Z, S, d, lo, hi = Z[cross], S[cross], d[cross], b0[cross], b1[cross]
    if Z.shape[0] == 0:
        return np.zeros(0), np.zeros(0)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        good = error_bound(Z, S, mid, d) <= eps64
        hi, lo = torch.where(good, mid, hi), torch.where(good, lo, mid)
    e64 = error_bound(Z, S, hi, d)
    e32 = error_bound(Z.float(), S.float(), hi.float()).to(F64)
    h = 1e-4
    slope = (torch.log(error_bound(Z, S, hi * (1 + h), d)) - torch.log(error_bound(Z, S, hi * (1 - h), d))) / (2 * h)
    return ((e32 - e64).abs() / e64).numpy(), slope.abs().numpy()
