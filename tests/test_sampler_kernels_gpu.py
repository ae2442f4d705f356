"""k_sampler_init / k_sampler_bound / k_sampler_resample (csrc/sampler.hip) driven directly through mp_sampler_*, on states this
file writes itself through hip.MpSamplerState: no network, no warp, no scene.

  * EXACT wherever the result is exactly specified: the stable merge, the sorts, the picks of the extras, flags, counters, and
    every row that must be left alone (the state's rows are followed by guard rows, and everything starts out poisoned).
  * RESIDUALS wherever the kernel takes a discrete decision from inexact arithmetic: the float64 reference
    (tests/sampler_reference.py) does not predict the device's output, it evaluates its own continuous function AT the device's
    output and the condition that defines the output must hold -- the bisection bracket contains a crossing of E64 = eps, and
    CDF64(z_device) = u.  Limits: tests/tolerances_sampler.py.
  * Every active ray of every case is asserted.  The only rays without a value check of their samples are the ones whose
    reference cdf is ill-conditioned (not `sharp`; fixed by the seeded generator, asserted on the CPU to be at most 13 of 37).

Shapes: 37 hit rays (not a multiple of the 4 waves of a workgroup) of a call of 40 rays in 5 convergence groups of 8; the
device-side hit count is 37, 29 (below the bound) or 50 (above it: clipped)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import sampler_reference as SR
from tests import tolerances_sampler as TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"
PF, PI = -7777.0, -77                       # poison of the float / int state
GUARD = 3
EPS32 = float(np.float32(SR.EPS))
TINY32 = float(np.float32(SR.ADD_TINY))
HIT = SR.hit_index()
GROUP_OF = HIT // SR.GROUP
COUNTS = (37, 29, 50)
WORST = {"E": 0.0, "cdf": 0.0}


def _hip():
    from multiply_amd import hip
    return hip


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    """bitwise equality (NaN-safe)"""
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


class Rig:
    """the state tensors of one sampler (poisoned, with GUARD rows past the rows in use), MpSamplerCfg / MpSamplerState, and the
    three launches as SamplerRun issues them"""

    def __init__(self, NS, NE, NX, J, iters, hit_count=SR.MAX_RAYS, max_rays=SR.MAX_RAYS, n_total=SR.N_TOTAL, hit=None,
                 far=None, near=SR.NEAR):
        hip = _hip()
        self.NS, self.NE, self.NX, self.J, self.iters = NS, NE, NX, J, iters
        self.max_rays, self.n_total, self.group = max_rays, n_total, SR.GROUP
        self.n_groups = (n_total + SR.GROUP - 1) // SR.GROUP
        self.zm, self.NF = NE * iters, NS + NX + 2
        self.n_eff = max(min(hit_count, max_rays), 0)
        rows = max(max_rays, 0) + GUARD
        f = lambda *s: torch.full(s, PF, dtype=torch.float32, device=DEV)
        i = lambda *s: torch.full(s, PI, dtype=torch.int32, device=DEV)
        self.t = dict(zs=f(rows, max(self.zm, 1)), sdfs=f(rows, max(self.zm, 1)), nz=i(rows), znew=f(rows, max(NE, 1)),
                      sdfnew=f(rows, max(NE, 1)), beta=f(rows), ray_active=i(rows),
                      group_flag=i((max(iters, 0) + 1) * self.n_groups + GUARD), zfinal=f(rows, max(self.NF, 1)),
                      iters=i(self.n_groups + GUARD), any_active=i(max(iters, 0) + 1 + GUARD))
        self.cfg = hip.MpSamplerCfg(NS, NE, NX, J, iters, SR.EPS, SR.ADD_TINY, near)
        self.state = hip.MpSamplerState(*[self.t[k].data_ptr() for k in ("zs", "sdfs", "nz", "znew", "sdfnew", "beta",
                                                                          "ray_active", "group_flag", "zfinal", "iters",
                                                                          "any_active")])
        self.hit_np = HIT if hit is None else hit
        self.far_np = SR.far_table() if far is None else far
        self.hit = torch.from_numpy(np.concatenate([self.hit_np, np.zeros(GUARD, np.int32)])).to(DEV)
        self.far = torch.from_numpy(self.far_np).to(DEV)
        self.count = torch.tensor([hit_count], dtype=torch.int32, device=DEV)
        self.beta0 = torch.zeros(1, dtype=torch.float32, device=DEV)

    def put(self, name, rows, value):
        """rows [0, len) of a state tensor <- a numpy array (columns [0, value.shape[1]) of 2-D tensors)"""
        v = torch.from_numpy(np.ascontiguousarray(value)).to(DEV)
        if v.dim() == 2:
            self.t[name][:rows, :v.shape[1]] = v
        else:
            self.t[name][:rows] = v

    def snap(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy().copy() for k, v in self.t.items()}

    def init(self, t_rand=None):
        hip = _hip()
        return hip.lib().mp_sampler_init(C.byref(self.cfg), C.byref(self.state), self.far, self.hit, self.count,
                                         self.max_rays, self.group, self.n_total, t_rand, hip.stream())

    def bound(self, beta0, it):
        hip = _hip()
        self.beta0.fill_(float(beta0))
        return hip.lib().mp_sampler_bound(C.byref(self.cfg), C.byref(self.state), self.beta0, self.hit, self.count,
                                          self.max_rays, self.group, self.n_total, it, hip.stream())

    def resample(self, beta0, it, u_final=None, extra_idx=None):
        hip = _hip()
        self.beta0.fill_(float(beta0))
        return hip.lib().mp_sampler_resample(C.byref(self.cfg), C.byref(self.state), self.beta0, self.far, self.hit,
                                             self.count, self.max_rays, self.group, self.n_total, it, u_final, extra_idx,
                                             hip.stream())


def _active(n_eff):
    """the rays a bound / resample launch must process: below the device count and with ray_active set"""
    a = np.ones(SR.MAX_RAYS, bool)
    a[list(SR.INACTIVE)] = False
    a[n_eff:] = False
    return a


def _assert_untouched(before, after, names, rows):
    """rows (a boolean mask over the first MAX_RAYS rows; the guard rows are always included) of the named tensors are unchanged"""
    for name in names:
        m = np.concatenate([rows, np.ones(before[name].shape[0] - rows.shape[0], bool)])
        assert same(before[name][m], after[name][m]), f"{name}: a row that must be left alone changed"


# ================================================================================================ init
def _check_init(rig, before, after, t_rand):
    R, NE, n = rig.max_rays, rig.NE, rig.n_eff
    far = rig.far_np[rig.hit_np[:n]]
    tr = None if t_rand is None else t_rand[:n].cpu().to(SR.F64)
    z64, _ = SR.init_depths(SR.NEAR, torch.from_numpy(far).to(SR.F64), NE, tr, EPS32)
    z = after["znew"][:n, :NE]
    err_ulp = np.abs(z.astype(np.float64) - z64.numpy()) / SR.ulp32(far)[:, None]
    b64 = SR.beta_init(torch.from_numpy(z).to(SR.F64), EPS32).numpy()
    err_beta = np.abs(after["beta"][:n].astype(np.float64) - b64) / b64
    print(f"init NE {NE}: znew {err_ulp.max():.2f} ulp(far), beta {err_beta.max():.2e} relative")
    assert err_ulp.max() <= TOL.INIT_Z_ULPS
    assert err_beta.max() <= TOL.INIT_BETA_REL
    assert (after["nz"][:n] == 0).all() and (after["ray_active"][:n] == 1).all()
    past = np.arange(R) >= n
    for name in ("znew", "beta", "nz", "ray_active"):
        m = np.concatenate([past, np.ones(GUARD, bool)])
        assert same(before[name][m], after[name][m]), name
    for name in ("zs", "sdfs", "sdfnew", "zfinal", "iters"):
        assert same(before[name], after[name]), name
    nflag = (rig.iters + 1) * rig.n_groups
    assert (after["group_flag"][:nflag] == 0).all() and (after["group_flag"][nflag:] == PI).all()
    assert after["any_active"][:rig.iters + 1].tolist() == [1] + [0] * rig.iters
    assert (after["any_active"][rig.iters + 1:] == PI).all()


@pytest.mark.parametrize("hit_count", COUNTS)
@pytest.mark.parametrize("jitter", [False, True], ids=["eval", "t_rand"])
@pytest.mark.parametrize("NE", [2, 63, 64, 65, 128, 256])
def test_init(NE, jitter, hit_count):
    rig = Rig(64, NE, 32, 10, 5, hit_count=hit_count)
    t_rand = torch.rand(SR.MAX_RAYS, NE, generator=torch.Generator().manual_seed(NE)).to(DEV) if jitter else None
    before = rig.snap()
    assert rig.init(t_rand) == 0
    _check_init(rig, before, rig.snap(), t_rand)


def test_init_grid_stride():
    """9 000 rays: more than the 2048 workgroups x 4 waves of the capped grid own one each"""
    R, total = 9000, 9016
    g = np.random.default_rng(5)
    hit = np.sort(g.choice(total, R, replace=False)).astype(np.int32)
    far = g.uniform(4.0, 6.0, total).astype(np.float32)
    rig = Rig(64, 64, 32, 10, 5, hit_count=R, max_rays=R, n_total=total, hit=hit, far=far)
    t_rand = torch.rand(R, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    before = rig.snap()
    assert rig.init(t_rand) == 0
    _check_init(rig, before, rig.snap(), t_rand)


# ================================================================================================ bound
@functools.lru_cache(maxsize=None)
def _bound_case(NE, n_old, beta0, family):
    case = SR.bound_case(NE, n_old, beta0, family, SR.case_seed("bound", NE, n_old, beta0, family))
    Z, S = SR.merged(case)
    case["Z64"], case["S64"], case["D64"] = Z, S, SR.d_star(Z, S)
    f32 = {k: torch.from_numpy(case[k]) for k in ("z_old", "s_old", "z_new", "s_new")}
    Z32, S32 = SR.merge(f32["z_old"], f32["s_old"], f32["z_new"], f32["s_new"])        # exact in any precision
    case["Z32"], case["S32"] = Z32.numpy(), S32.numpy()
    return case


@functools.lru_cache(maxsize=None)
def _run_bound(NE, n_old, beta0, family, iters, J, it, hit_count):
    case = _bound_case(NE, n_old, beta0, family)
    assert n_old + NE <= NE * iters
    rig = Rig(64, NE, 32, J, iters, hit_count=hit_count)
    R = SR.MAX_RAYS
    rig.put("zs", R, case["z_old"]); rig.put("sdfs", R, case["s_old"])
    rig.put("nz", R, np.full(R, n_old, np.int32))
    rig.put("znew", R, case["z_new"]); rig.put("sdfnew", R, case["s_new"])
    rig.put("beta", R, case["beta_prev"])
    act = np.ones(R, np.int32)
    act[list(SR.INACTIVE)] = 0
    rig.put("ray_active", R, act)
    rig.t["group_flag"][:(iters + 1) * rig.n_groups] = 0
    before = rig.snap()
    assert rig.bound(case["beta0"], it) == 0
    return rig, case, before, rig.snap()


def _check_merge(rig, case, before, after):
    n = case["n_old"] + case["NE"]
    act = _active(rig.n_eff)
    for k in np.nonzero(act)[0]:
        assert same(after["zs"][k, :n], case["Z32"][k]), f"ray {k}: depths are not the stable merge"
        assert same(after["sdfs"][k, :n], case["S32"][k]), f"ray {k}: sdf values are not in the stable merge's order"
        assert same(after["zs"][k, n:], before["zs"][k, n:]) and same(after["sdfs"][k, n:], before["sdfs"][k, n:])
        assert after["nz"][k] == n
    _assert_untouched(before, after, ("zs", "sdfs", "nz", "beta"), ~act)
    _assert_untouched(before, after, ("znew", "sdfnew", "ray_active", "zfinal"), np.ones(SR.MAX_RAYS, bool))
    assert same(before["iters"], after["iters"]) and same(before["any_active"], after["any_active"])


def _check_line_search(rig, case, before, after, it):
    J, dE = rig.J, TOL.DELTA_E
    Z, S, D = case["Z64"], case["S64"], case["D64"]
    E = lambda beta: SR.error_bound(Z, S, torch.as_tensor(beta, dtype=SR.F64), D).numpy()
    b0 = float(case["beta0"])
    bp32, out32 = before["beta"][:SR.MAX_RAYS], after["beta"][:SR.MAX_RAYS]
    bp, out = bp32.astype(np.float64), out32.astype(np.float64)
    w = (bp - b0) / 2.0 ** J
    low = out * (1.0 - 2.0 ** -22) if J == 30 else out - w
    E0, Eout, Elow = E(b0), E(out), E(np.maximum(low, b0))
    act = _active(rig.n_eff)
    at_b0 = _bits(out32) == _bits(np.full_like(out32, case["beta0"]))
    n_b0 = n_search = 0

    def le(e, k, what):       # E64 <= eps within DELTA_E
        WORST["E"] = max(WORST["E"], e / EPS32 - 1.0)
        assert e <= EPS32 * (1 + dE), f"ray {k}: {what}: E64 {e:.9g} > eps"

    def ge(e, k, what):       # E64 >= eps within DELTA_E
        WORST["E"] = max(WORST["E"], 1.0 - e / EPS32)
        assert e >= EPS32 * (1 - dE), f"ray {k}: {what}: E64 {e:.9g} < eps"

    for k in np.nonzero(act)[0]:
        if k == SR.NAN_RAY:                                    # a NaN bound satisfies neither comparison: beta stays
            assert same(out32[k:k + 1], bp32[k:k + 1]), "the ray with a NaN sdf must keep its beta"
            continue
        if at_b0[k]:
            n_b0 += 1
            le(E0[k], k, "beta0 was returned")
            continue
        n_search += 1
        ge(E0[k], k, "the search was entered")
        if not same(out32[k:k + 1], bp32[k:k + 1]):
            le(Eout[k], k, "the returned beta was accepted")
        assert b0 < out[k] <= bp[k]
        if J >= 1:
            ge(Elow[k], k, "the lower end of the bracket was rejected")
        if 1 <= J <= 10:
            m = (out[k] - b0) / w[k]
            assert abs(m - round(m)) <= TOL.LATTICE and 1 <= round(m) <= 2 ** J, f"ray {k}: {m} steps of the bisection lattice"
    # the convergence vote: row `it` of the flag table, one flag per group with a ray above beta0; every other row stays 0
    want = np.zeros((rig.iters + 1, rig.n_groups), np.int32)
    for k in np.nonzero(act)[0]:
        if out32[k] > case["beta0"]:
            want[it, GROUP_OF[k]] = 1
    nflag = want.size
    assert after["group_flag"][:nflag].reshape(want.shape).tolist() == want.tolist()
    assert (after["group_flag"][nflag:] == PI).all()
    if act[SR.NAN_RAY]:
        assert after["group_flag"][it * rig.n_groups + GROUP_OF[SR.NAN_RAY]] == 1
    return n_b0, n_search


@pytest.mark.parametrize("hit_count", COUNTS)
@pytest.mark.parametrize("m_old", [0, 1, 3])
@pytest.mark.parametrize("NE", [2, 64, 65, 128])
def test_bound_merge(NE, m_old, hit_count):
    """(zs, sdfs)[:n] is bit for bit the stable merge (old before new on equal depth; the states hold such ties on purpose),
    nz == n, inactive rows and rows at or beyond the device count are untouched"""
    rig, case, before, after = _run_bound(NE, m_old * NE, 0.01, "random", 5, 0, 1, hit_count)
    _check_merge(rig, case, before, after)
    _check_line_search(rig, case, before, after, 1)


LS_PARAMS = [(c, J, (2 if J == 10 else 0), COUNTS[(i + j) % 3])
             for i, c in enumerate(SR.LINE_SEARCH_CASES) for j, J in enumerate((0, 1, 10, 30))]
LS_PARAMS += [(SR.LINE_SEARCH_CASES[1], 10, 0, 37), (SR.LINE_SEARCH_CASES[2], 1, 2, 37)]


@pytest.mark.parametrize("c,J,it,hit_count", LS_PARAMS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bound_line_search(c, J, it, hit_count):
    """the returned beta brackets a crossing of E64 = eps (tests/tolerances_sampler.py DELTA_E) on every active ray, and the
    group flags of iteration `it` are those of the returned betas"""
    NE, n_old, beta0, family, iters = c
    rig, case, before, after = _run_bound(NE, n_old, beta0, family, iters, J, it, hit_count)
    _check_merge(rig, case, before, after)
    n_b0, n_search = _check_line_search(rig, case, before, after, it)
    print(f"line search {c} J {J}: {n_b0} rays at beta0, {n_search} searched; worst E residual so far {WORST['E']:.3e}")


# ================================================================================================ resample
FLAGGED = (1, 3)


@functools.lru_cache(maxsize=None)
def _resample_case(NE, n, iters, it, family, inverted=False):
    case = SR.resample_case(NE, n, SR.case_seed("inverted") if inverted else SR.case_seed("resample", NE, n, iters, it, family),
                            family, inverted)
    for more in (True, False):
        case["cdf", more] = SR.cdfs(case, more, SR.ADD_TINY).numpy()
        case["sharp", more] = SR.sharp_rays(case, more, SR.ADD_TINY)
    return case


@functools.lru_cache(maxsize=None)
def _run_resample(NE, n, iters, it, family, train, hit_count, NS=64, NX=32, inverted=False):
    case = _resample_case(NE, n, iters, it, family, inverted)
    assert n <= NE * iters and NS + NX + 2 <= NE * iters       # the list and the final set both fit a ray's row of LDS
    rig = Rig(NS, NE, NX, 10, iters, hit_count=hit_count)
    R = SR.MAX_RAYS
    rig.put("zs", R, case["Z"]); rig.put("sdfs", R, case["S"])
    rig.put("nz", R, np.full(R, n, np.int32))
    rig.put("beta", R, case["beta"])
    act = np.ones(R, np.int32)
    act[list(SR.INACTIVE)] = 0
    rig.put("ray_active", R, act)
    # the flags of iteration `it`: groups 1 and 3.  The rows before and after it hold the opposite pattern.
    flags = np.zeros((iters + 1, rig.n_groups), np.int32)
    flags[:, [g for g in range(rig.n_groups) if g not in FLAGGED]] = 1
    flags[it] = 0
    flags[it, list(FLAGGED)] = 1
    rig.put("group_flag", flags.size, flags.reshape(-1))
    u_final = extra_idx = None
    if train:
        g = torch.Generator().manual_seed(n + it)
        u_final = torch.rand(R, NS, generator=g).to(DEV)
        extra_idx = torch.stack([torch.randperm(NE * k, generator=g)[:NX] for k in range(1, iters + 1)]).to(torch.int32).to(DEV)
    before = rig.snap()
    assert rig.resample(0.01, it, u_final, extra_idx) == 0
    ctx = dict(train=train, it=it, u_final=None if u_final is None else u_final.cpu().numpy(),
               extra_idx=None if extra_idx is None else extra_idx.cpu().numpy())
    return rig, case, before, rig.snap(), ctx


def _continues(rig, it):
    """per hit ray: its group is flagged and another iteration is left"""
    return np.isin(GROUP_OF, FLAGGED) & (it + 1 < rig.iters)


def _check_bookkeeping(rig, case, before, after, ctx):
    it = ctx["it"]
    act, more = _active(rig.n_eff), _continues(rig, it)
    cont, fin = act & more, act & ~more
    for k in np.nonzero(cont)[0]:
        assert not same(after["znew"][k], before["znew"][k]), f"ray {k}: znew was not rewritten"
        assert after["ray_active"][k] == 1
    for k in np.nonzero(fin)[0]:
        assert not (_bits(after["zfinal"][k]) == _bits(np.float32(PF))).any(), f"ray {k}: zfinal has unwritten entries"
        assert after["ray_active"][k] == 0
    _assert_untouched(before, after, ("zfinal",), ~fin)
    _assert_untouched(before, after, ("znew",), ~cont)
    _assert_untouched(before, after, ("ray_active",), ~fin)
    _assert_untouched(before, after, ("zs", "sdfs", "nz", "beta", "sdfnew"), np.ones(SR.MAX_RAYS, bool))
    assert same(before["group_flag"], after["group_flag"])
    want_iters = before["iters"].copy()
    want_iters[np.unique(GROUP_OF[fin])] = it + 1
    assert after["iters"].tolist() == want_iters.tolist()
    want_any = before["any_active"].copy()
    if cont.any():
        want_any[it + 1] = 1
    assert after["any_active"].tolist() == want_any.tolist()
    if it + 1 == rig.iters:
        assert not cont.any() and fin.sum() == act.sum()        # every ray finalises, whatever its flag
    return cont, fin


def _remove_one(row, v):
    """row (float32, ascending) without ONE entry bitwise equal to v"""
    at = np.nonzero(_bits(row) == _bits(np.float32(v)))[0]
    assert at.size, f"the final set lacks {float(v)!r}"
    return np.delete(row, at[0])


def _final_samples(rig, case, after, ctx, k):
    """zfinal row k is ascending and holds near, far and the extras; -> the NS values that remain (ascending)"""
    n, row = case["n"], after["zfinal"][k]
    assert (row[1:] >= row[:-1]).all(), f"ray {k}: zfinal is not ascending"
    idx = ctx["extra_idx"][n // rig.NE - 1].astype(np.int64) if ctx["train"] else SR.extra_indices(n, rig.NX).numpy()
    rest = _remove_one(_remove_one(row, SR.NEAR), rig.far_np[HIT[k]])
    for v in case["Z"][k][idx]:
        rest = _remove_one(rest, v)
    assert rest.shape == (rig.NS,)
    return rest


def _check_final_set(rig, case, before, after, ctx):
    _, fin = _check_bookkeeping(rig, case, before, after, ctx)
    for k in np.nonzero(fin)[0]:
        _final_samples(rig, case, after, ctx, k)
    return fin


def _check_samples(rig, case, before, after, ctx, value_rays=None):
    """the samples: within [near, far] and ascending in u on every ray; on the sharp rays u_j lies within DELTA_CDF (+ the
    rounding of the depth) of the float64 cdf at the returned depth"""
    cont, fin = _check_bookkeeping(rig, case, before, after, ctx)
    n_value = 0
    for k in np.nonzero(cont | fin)[0]:
        more = bool(cont[k])
        if more:
            z = after["znew"][k, :rig.NE]
            u = np.linspace(0.0, 1.0, rig.NE)
        else:
            z = _final_samples(rig, case, after, ctx, k)
            u = np.sort(ctx["u_final"][k].astype(np.float64)) if ctx["train"] else np.linspace(0.0, 1.0, rig.NS)
        far = rig.far_np[HIT[k]]
        assert (z >= SR.NEAR).all() and (z <= far).all(), f"ray {k}: a sample outside [near, far]"
        assert (z[1:] >= z[:-1]).all(), f"ray {k}: samples are not ascending in u"
        if not case["sharp", more][k] or (value_rays is not None and not value_rays[k]):
            continue
        n_value += 1
        F_lo, F_hi, slope = SR.cdf_interval(case["Z"][k], case["cdf", more][k], z)
        dist = np.maximum(np.maximum(F_lo - u, u - F_hi), 0.0) - 4.0 * SR.ulp32(z) * slope
        WORST["cdf"] = max(WORST["cdf"], float(dist.max()))
        j = int(dist.argmax())
        assert dist[j] <= TOL.DELTA_CDF, (f"ray {k} ({'more' if more else 'final'}), sample {j}: u {u[j]:.8f} is {dist[j]:.3e} "
                                          f"from cdf64(z) [{F_lo[j]:.8f}, {F_hi[j]:.8f}]")
    return n_value


RES_PARAMS = [(c, train, 37) for c in SR.RESAMPLE_CASES for train in (False, True)]
RES_PARAMS += [(SR.RESAMPLE_CASES[0], False, 29), (SR.RESAMPLE_CASES[0], True, 50), (SR.RESAMPLE_CASES[1], False, 50),
               (SR.RESAMPLE_CASES[1], True, 29)]
_res_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("c,train,hit_count", RES_PARAMS, ids=_res_ids)
def test_resample_bookkeeping(c, train, hit_count):
    """who continues (flagged group, iterations left: znew rewritten, any_active[iter+1], still active) and who finalises (zfinal,
    ray_active 0, iters[grp] = iter + 1); at the last iteration everybody; nothing else changes"""
    NE, n, iters, it, family = c
    rig, case, before, after, ctx = _run_resample(NE, n, iters, it, family, train, hit_count)
    cont, fin = _check_bookkeeping(rig, case, before, after, ctx)
    assert fin.any() and (cont.any() or it + 1 == iters)


@pytest.mark.parametrize("c,train,hit_count", RES_PARAMS, ids=_res_ids)
def test_resample_final_set(c, train, hit_count):
    """every zfinal row is ascending and holds, bit for bit, near, far and the N_extra picks Z[idx] (eval: torch's own
    linspace(0, n-1, NX).long(); training: row n/NE - 1 of extra_idx) next to its N samples"""
    NE, n, iters, it, family = c
    rig, case, before, after, ctx = _run_resample(NE, n, iters, it, family, train, hit_count)
    assert _check_final_set(rig, case, before, after, ctx).any()


@pytest.mark.parametrize("c,train,hit_count", RES_PARAMS, ids=_res_ids)
def test_resample_samples(c, train, hit_count):
    NE, n, iters, it, family = c
    rig, case, before, after, ctx = _run_resample(NE, n, iters, it, family, train, hit_count)
    n_value = _check_samples(rig, case, before, after, ctx)
    print(f"resample {c} train {train}: {n_value} rays value-checked; worst cdf residual so far {WORST['cdf']:.3e}")
    assert n_value >= min(24, _active(rig.n_eff).sum() - 13)


def test_resample_unordered_samples_take_the_fallback_sort():
    """eval mode, but the inverse-cdf samples of every other ray come out unordered by one float32 step (their lists carry one
    adjacent pair of depths swapped by that step; test_sampler_reference_cpu.py shows the reference's own float32 samples
    unordered): the sorted-run fast path must not be taken and the row must still come out ascending, with the right
    members.  On those rays the list is not ascending, so there is no piecewise-linear cdf to evaluate: they get the exact
    checks; the other rays are value-checked as everywhere."""
    NE, NS, NX = SR.INVERTED_NE, SR.INVERTED_NS, SR.INVERTED_NX
    rig, case, before, after, ctx = _run_resample(NE, NE, 5, 4, "sphere", False, 37, NS, NX, True)
    fin = _check_final_set(rig, case, before, after, ctx)
    assert fin.sum() == _active(37).sum()
    ordered = np.arange(SR.MAX_RAYS) % 2 == 0
    _check_samples(rig, case, before, after, ctx, value_rays=ordered)


# ================================================================================================ the large-list paths
@pytest.mark.parametrize("c", SR.LARGE_BOUND_CASES, ids=_res_ids)
def test_large_lists_bound(c):
    """n = 768 and 1024 > MAXCH * 64 = 640: the error bound from LDS (80 KiB of dynamic LDS), which the shipped configuration
    never reaches"""
    NE, n_old, beta0, family, iters = c
    rig, case, before, after = _run_bound(NE, n_old, beta0, family, iters, 10, 3, 37)
    _check_merge(rig, case, before, after)
    n_b0, n_search = _check_line_search(rig, case, before, after, 3)
    print(f"large bound {c}: {n_b0} rays at beta0, {n_search} searched; worst E residual so far {WORST['E']:.3e}")


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("c", SR.LARGE_RESAMPLE_CASES, ids=_res_ids)
def test_large_lists_resample(c, train):
    """the same lists through the resampling kernel's recompute path (chunks of more than MAXCH samples per lane)"""
    NE, n, iters, it, family = c
    rig, case, before, after, ctx = _run_resample(NE, n, iters, it, family, train, 37)
    _check_final_set(rig, case, before, after, ctx)
    n_value = _check_samples(rig, case, before, after, ctx)
    print(f"large resample {c} train {train}: {n_value} rays value-checked; worst cdf residual so far {WORST['cdf']:.3e}")
    assert n_value >= 24


# ================================================================================================ argument errors
BAD_CFG = [dict(NE=1), dict(NE=257), dict(NS=0), dict(iters=0), dict(iters=9)]


@pytest.mark.parametrize("bad", BAD_CFG, ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_bad_cfg_is_refused(bad):
    kw = dict(NS=64, NE=64, NX=32, J=10, iters=5)
    kw.update(bad)
    rig = Rig(kw["NS"], kw["NE"], kw["NX"], kw["J"], kw["iters"])
    before = rig.snap()
    for call in (lambda: rig.init(None), lambda: rig.bound(0.01, 0), lambda: rig.resample(0.01, 0)):
        with pytest.raises(RuntimeError, match=r"failed with code -1$"):        # hip.check on the entry point's status
            call()
    after = rig.snap()
    assert all(same(before[k], after[k]) for k in before)


@pytest.mark.parametrize("max_rays", [0, -3])
def test_no_rays_launches_nothing(max_rays):
    rig = Rig(64, 64, 32, 10, 5, hit_count=37, max_rays=max_rays)
    before = rig.snap()
    assert rig.init(None) == 0 and rig.bound(0.01, 0) == 0 and rig.resample(0.01, 0) == 0
    after = rig.snap()
    assert all(same(before[k], after[k]) for k in before)
