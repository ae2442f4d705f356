"""tests/sampler_reference.py pinned to the oracle, and the conditions its generated inputs must meet.

1. The staged float64 reference, chained, reproduces oracle.multiply_oracle.error_bound_sample (run under a float64 default
   dtype) on an analytic SDF: the same iteration count, depths equal to 1e-12, for eval draws and for training draws.
2. The input conditions the GPU file (tests/test_sampler_kernels_gpu.py) relies on hold on the reference alone: the gap
   beta_prev - beta0, the coverage of the three d* branches, the beta0 values, the number of sharp rays, and the CPU spreads
   recorded in tests/tolerances_sampler.py.  A generator change that breaks one fails here, not on the GPU."""
import numpy as np
import pytest
import torch

from oracle import multiply_oracle as O
from tests import sampler_reference as SR
from tests import tolerances_sampler as TOL


@pytest.fixture
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(old)


def _sphere_rays():
    """rays from distance 3 at a sphere of radius 0.6, impact parameters 0 .. 0.9"""
    b = torch.linspace(0.0, 0.9, SR.MAX_RAYS, dtype=torch.float64)
    sin = b / SR.CAM_DIST
    dirs = torch.stack([sin, torch.zeros_like(sin), torch.sqrt(1.0 - sin ** 2)], -1)
    cam = torch.tensor([0.0, 0.0, -SR.CAM_DIST], dtype=torch.float64)[None].repeat(SR.MAX_RAYS, 1)
    return dirs, cam


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("NE,NS,NX,beta0", [(64, 64, 32, 0.01), (32, 16, 8, 0.1), (65, 33, 7, 0.003)])
def test_chain_reproduces_the_oracle(float64_default, train, NE, NS, NX, beta0):
    dirs, cam = _sphere_rays()
    R = dirs.shape[0]
    cfg = O.SamplerCfg(N_samples=NS, N_samples_eval=NE, N_samples_extra=NX, eps=0.1, beta_iters=10, max_total_iters=5,
                       add_tiny=1e-6, near=0.0, radius=SR.BOUND_R)
    draws = None
    if train:
        g = torch.Generator().manual_seed(3)
        draws = dict(t_rand=torch.rand(R, NE, generator=g, dtype=torch.float64),
                     u_final=torch.rand(R, NS, generator=g, dtype=torch.float64),
                     extra_idx=torch.stack([torch.randperm(NE * k, generator=g)[:NX] for k in range(1, 6)]))

    def sdf_points(p):
        return p.norm(dim=-1, keepdim=True) - SR.SPHERE_R

    def sdf_of_z(z):
        return sdf_points((cam[:, None, :] + z[:, :, None] * dirs[:, None, :]).reshape(-1, 3)).reshape(z.shape)

    want, want_it = O.error_bound_sample(cfg, dirs, cam, sdf_points, beta0, draws)
    far = O.sphere_far(cam, dirs, cfg.radius)[:, 0]
    got, got_it = SR.run_chain(cfg, cfg.near, far, sdf_of_z, beta0, draws)
    assert got.dtype == torch.float64 and want.dtype == torch.float64
    assert got_it == want_it
    assert got_it > 1, "the chain must resample at least once for this to pin the up-sampling stages"
    assert got.shape == want.shape == (R, NS + NX + 2)
    assert float((got - want).abs().max()) <= 1e-12


def test_cdf_interval():
    Z = np.array([0.0, 1.0, 1.0, 1.0, 2.0, 4.0])
    cdf = np.array([0.0, 0.2, 0.3, 0.5, 0.6, 1.0])
    lo, hi, slope = SR.cdf_interval(Z, cdf, np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]))
    assert np.allclose(lo, [0.0, 0.1, 0.2, 0.55, 0.6, 0.8, 1.0])
    assert np.allclose(hi, [0.0, 0.1, 0.5, 0.55, 0.6, 0.8, 1.0])
    assert np.allclose(slope, [0.2, 0.2, 0.2, 0.1, 0.2, 0.2, 0.2])


def test_merge_is_stable_and_extras_are_torchs():
    zo, so = torch.tensor([[0.0, 1.0, 1.0, 3.0]]), torch.tensor([[10.0, 11.0, 12.0, 13.0]])
    zn, sn = torch.tensor([[0.0, 1.0, 2.0]]), torch.tensor([[20.0, 21.0, 22.0]])
    Z, S = SR.merge(zo, so, zn, sn)
    assert Z.tolist() == [[0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 3.0]]
    assert S.tolist() == [[10.0, 20.0, 11.0, 12.0, 21.0, 22.0, 13.0]]
    assert SR.extra_indices(320, 32).tolist() == torch.linspace(0, 319, 32).long().tolist()


# ------------------------------------------------------------------------------------------------ input conditions
BOUND_CASES = SR.LINE_SEARCH_CASES + SR.LARGE_BOUND_CASES
RES_CASES = SR.RESAMPLE_CASES + SR.LARGE_RESAMPLE_CASES


def _bound(c):
    return SR.bound_case(*c[:4], SR.case_seed("bound", *c[:4]))


def test_line_search_inputs_meet_their_conditions():
    counts, total = np.zeros(3), 0
    converged = searched = 0
    for c in BOUND_CASES:
        case = _bound(c)
        assert case["z_old"].shape[1] + c[0] <= c[0] * c[4], "the merged list must fit the state's rows"
        assert ((case["beta_prev"].astype(np.float64) - case["beta0"]) >= 0.01 * case["beta0"]).all()
        Z, S = SR.merged(case)
        assert (Z[:, 1:] >= Z[:, :-1]).all()
        assert int((Z[:, 1:] == Z[:, :-1]).sum()) >= SR.MAX_RAYS, "ties are part of the cases"
        ok = ~torch.isnan(S).any(-1)
        assert int((~ok).sum()) == 1 and not bool(ok[SR.NAN_RAY])
        br = SR.d_star_branches(Z[ok], S[ok])
        counts += [int(m.sum()) for m in br]
        total += br[0].numel()
        e0 = SR.error_bound(Z[ok], S[ok], float(case["beta0"]))
        converged += int((e0 <= SR.EPS).sum())
        searched += int((e0 > SR.EPS).sum())
    frac = counts / total
    print("d* branches (first, second, Heron):", frac)
    assert (frac >= 0.005).all(), frac
    assert {float(np.float32(c[2])) for c in SR.LINE_SEARCH_CASES} == {float(np.float32(x)) for x in (0.1, 0.01, 0.001)}
    assert converged >= 50 and searched >= 50, (converged, searched)     # both outcomes of the first test occur


def test_cpu_spread_of_the_error_bound_is_the_recorded_one():
    worst, slopes = 0.0, []
    for c in BOUND_CASES:
        sp, sl = SR.root_spread(_bound(c))
        if len(sp):
            worst = max(worst, float(sp.max()))
            slopes += sl.tolist()
    print(f"CPU_SPREAD_E {worst:.3e}  |d ln E / d ln beta| {min(slopes):.2f} .. {max(slopes):.2f} over {len(slopes)} roots")
    assert len(slopes) >= 50
    assert 0.5 * TOL.CPU_SPREAD_E <= worst <= 1.1 * TOL.CPU_SPREAD_E
    assert max(slopes) <= 8.3          # what the factor 16 of DELTA_E allows for


def test_resample_inputs_are_sharp_and_conditioned():
    worst = 0.0
    for c in RES_CASES:
        NE, n, iters, it, fam = c
        assert n <= NE * iters
        case = SR.resample_case(NE, n, SR.case_seed("resample", *c), fam)
        again = SR.resample_case(NE, n, SR.case_seed("resample", *c), fam)
        assert all(np.array_equal(case[k], again[k]) for k in ("Z", "S", "beta"))          # seeded: the sharp set is fixed
        assert (np.diff(case["Z"].astype(np.float64), axis=-1) > 0).all(), "distinct depths identify the picks"
        assert set(case["beta"].tolist()) == {float(np.float32(x)) for x in SR.RESAMPLE_BETAS}
        for more in (True, False):
            spread = SR.cdf_spread(case, more, SR.ADD_TINY)
            sharp = SR.sharp_rays(case, more, SR.ADD_TINY)
            assert int(sharp.sum()) >= 24, (c, more, int(sharp.sum()))
            assert sharp[case["b"] <= 0.5].all(), "rays through the sphere are sharp"
            worst = max(worst, float(spread[sharp].max()))
    print(f"CPU_SPREAD_CDF {worst:.3e}")
    assert 0.5 * TOL.CPU_SPREAD_CDF <= worst <= 1.1 * TOL.CPU_SPREAD_CDF


def test_inverted_state_is_what_the_fallback_case_needs():
    case = SR.resample_case(8, 8, SR.case_seed("inverted"), inverted=True)
    d = np.diff(case["Z"].astype(np.float64), axis=-1)
    assert (d[0::2] > 0).all() and ((d[1::2] < 0).sum(-1) == 1).all()
    assert np.abs(d[1::2][d[1::2] < 0]).max() <= SR.ulp32(case["far"]).max()
    # the reference's own float32 inverse cdf of these rays comes out unordered, by that one step
    cdf = SR.cdfs(case, False, SR.ADD_TINY, torch.float32)
    u = torch.linspace(0.0, 1.0, SR.INVERTED_NS)[None].repeat(SR.MAX_RAYS, 1)
    z = SR.inverse_cdf(torch.from_numpy(case["Z"]), cdf, u).numpy().astype(np.float64)
    dz = np.diff(z, axis=-1)
    assert (dz[0::2] >= 0).all() and (dz[1::2] < 0).any(-1).all()
    assert dz.min() >= -2 * SR.ulp32(case["far"]).max()
