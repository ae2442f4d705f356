"""Registration on the device (multiply_amd/registration.py, csrc/registration.hip) against the float64 reference
(tests/registration_reference.py): the four entry points on arrays the tests write, one ICP step in lockstep with the reference on
the device's own correspondences, and the loop end to end on the shapes of tests/registration_shapes.py.

The end-to-end bound ("the exact-copy bound"): max_v |T v - T0 v| <= 4 x 16 FLT_EPSILON M, M the largest |coordinate| of the two
meshes.  16 FLT_EPSILON M is the stated slack of the closest query, whose fp32 closest points are the data the
iteration fits; 4 is the margin.  No end state is compared between different tessellations (a limit cycle)."""
import numpy as np
import pytest
import torch

from multiply_amd import registration as reg
from tests import mesh_metrics_reference as MR
from tests import registration_reference as RR
from tests import registration_shapes as RS

pytestmark = pytest.mark.gpu

EPS, FLT_EPSILON = 2.0 ** -52, 2.0 ** -23
SIZES = (0, 1, 63, 64, 65, 257, 4099)
AXIS = (1.0, 2.0, -1.0)


def exact_copy_bound(*verts):
    return 4 * 16 * FLT_EPSILON * max(float(np.abs(v).max()) for v in verts)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def poisoned(a, pad=8):
    """the array on the device in the middle of a NaN-filled (255 for bytes / -1 for ints) buffer: (view, buffer)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    n = t.shape[0]
    fill = float("nan") if t.dtype.is_floating_point else (255 if t.dtype == torch.uint8 else -1)
    buf = torch.full((n + 2 * pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype).cuda()
    buf[pad:pad + n] = t.cuda()
    return buf[pad:pad + n], buf


def half_ulp32(x):
    """half a unit in the last place of the fp32 binade of |x| (float64 in, float64 out)"""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - 25)


# ------------------------------------------------------------------------------------------------ mp_reg_apply
@pytest.mark.parametrize("n", SIZES)
def test_apply_forward_and_inverse_against_float64(n):
    from multiply_amd import hip
    rng = np.random.RandomState(10 + n)
    st = RR.new_state(0.83, RS.rotation(AXIS, 37.0), [0.4, -1.3, 2.1], [-1, -1, -1], [1, 1, 1])
    p = (rng.normal(0, 1, (n, 3)) * 1.5 + [0.5, -0.2, 3.0]).astype(np.float32)
    state = dev(st)
    pd, buf = poisoned(p)
    fwd = hip.reg_apply(pd, state)
    inv = hip.reg_apply(pd, state, inverse=True)
    back = hip.reg_apply(fwd, state, inverse=True)
    assert fwd.shape == (n, 3) and torch.isnan(buf[:8]).all() and torch.isnan(buf[8 + n:]).all()
    if n == 0:
        return
    for name, got, want in (("forward", fwd, RR.apply(st, p)), ("inverse", inv, RR.apply(st, p, inverse=True))):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        tol = half_ulp32(want) * (1 + 1e-6) + 1e-15      # one rounding to fp32 of a double that carries ~10 roundings of its own
        print(f"[apply {name} n={n}] worst error / half an fp32 ulp: {(err / half_ulp32(want)).max():.4f}")
        assert (err <= tol).all()
    M = max(np.abs(p).max(), np.abs(fwd.cpu().numpy()).max())
    ulp = 2 * half_ulp32(M)
    e = np.abs(back.cpu().numpy().astype(np.float64) - p).max()
    print(f"[apply inverse o forward n={n}] {e / ulp:.3f} ulp of the largest coordinate {M:.3f}")
    assert e <= 2 * ulp


# ------------------------------------------------------------------------------------------------ mp_reg_rows
def dyadic_pairs(n, seed, in_source):
    """Pairs whose every term is EXACT in double, so that the device and the reference differ by the order of the sums alone (the
    bound n 2^-52 sum |terms| is a bound on summation): coordinates on the 2^-10 grid, normals on the 2^-8 grid (unit to 2^-8),
    s = 1, R a signed permutation, t and c on the grid -- a row entry has at most 25 bits, a product of two at most 50.  tau2 =
    0.5625; an accepted pair has d2 <= 0.1875, a rejected one d2 >= 1: far off tau2.  Every eleventh pair is non-finite somewhere."""
    rng = np.random.RandomState(seed)
    grid = lambda lo, hi, size, bits: rng.randint(int(lo * 2 ** bits), int(hi * 2 ** bits) + 1, size) / 2.0 ** bits
    Rm = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])
    st = RR.new_state(1.0, Rm, [0.25, -0.5, 0.125], [-1.5, -2.0, -1.0], [2.0, 1.5, 1.25], tau2=0.5625)
    p = grid(-2, 2, (n, 3), 10)
    x = p @ Rm.T + st[RR.T:RR.T + 3]
    e = grid(-0.25, 0.25, (n, 3), 10)
    far = rng.uniform(0, 1, n) < 0.3
    e[far, rng.randint(0, 3, n)[far]] = rng.choice([-1.5, 1.25, 1.0], int(far.sum()))
    q = x + e
    u = rng.normal(0, 1, (n, 3))
    nrm = np.round(u / np.linalg.norm(u, axis=1, keepdims=True) * 256) / 256
    bad = np.arange(n) % 11 == 5
    for k in np.nonzero(bad)[0]:
        [p, q, nrm][k % 3][k, k % 2] = [np.nan, np.inf, -np.inf][k % 3]
    arrays = [a.astype(np.float32) for a in (p, q, nrm)]
    assert all(np.array_equal(a.astype(np.float64)[~bad], b[~bad]) for a, b in zip(arrays, (p, q, nrm)))       # exact in fp32
    return st, arrays, far & ~bad, bad


@pytest.mark.parametrize("in_source", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_rows_against_float64(n, in_source):
    from multiply_amd import hip
    st, (p, q, nrm), far, bad = dyadic_pairs(n, 100 + n, in_source)
    want, want_mask, terms = RR.rows(p, q, nrm, st, in_source)
    with np.errstate(all="ignore"):
        d2 = ((RR.apply(st, p) - q.astype(np.float64)) ** 2).sum(1)
    assert ((want_mask == 1) == far).all() and ((want_mask == 2) == bad).all()
    assert (d2[want_mask == 0] <= 0.1875).all() and (d2[want_mask == 1] >= 1).all()        # tau2 = 0.5625
    state = dev(st)
    (pd, pb), (qd, qb), (nd, nb) = poisoned(p), poisoned(q), poisoned(nrm)
    md, mb = poisoned(np.full(n, 7, np.uint8))
    slots = torch.full((3, hip.REG_SLOT), float("nan"), dtype=torch.float64, device="cuda")
    work = hip.reg_work("cuda")
    hip.reg_rows(pd, qd, nd, state, slots[1], normals_in_source=in_source, work=work, mask=md)
    got = slots[1].cpu().numpy().copy()
    work.fill_(float("nan"))
    hip.reg_rows(pd, qd, nd, state, slots[1], normals_in_source=in_source, work=work)
    assert np.array_equal(got, slots[1].cpu().numpy()), "two calls differ in bits"
    assert torch.isnan(slots[0]).all() and torch.isnan(slots[2]).all()
    assert np.array_equal(md.cpu().numpy(), want_mask) and (mb[:8] == 255).all() and (mb[8 + n:] == 255).all()
    for k in (RR.N_ACC, RR.N_REJ, RR.N_OUT):
        assert got[k] == want[k]
    assert got[RR.N_ACC] + got[RR.N_REJ] + got[RR.N_OUT] == n
    bound = n * EPS * np.abs(terms).sum(0)
    off = np.abs(got - want)
    worst = (off[:37] / np.where(bound[:37] > 0, bound[:37], 1)).max() if n else 0.0
    print(f"[rows n={n} in_source={in_source}] accepted {got[RR.N_ACC]:.0f} rejected {got[RR.N_REJ]:.0f} left out {got[RR.N_OUT]:.0f}; "
          f"worst |sum - float64| / (n 2^-52 sum|terms|) = {worst:.3e}")
    assert (off <= bound).all()
    # the same pairs through a face list: ids into a table of normals, out-of-range ids are left out
    if n:
        fin_n = np.isfinite(nrm).all(1)
        table = np.concatenate([nrm[fin_n], np.zeros((1, 3), np.float32)])
        face = np.full(n, -1, np.int32)
        face[fin_n] = np.arange(int(fin_n.sum()))
        face[~fin_n] = [-1, table.shape[0]][n % 2]
        hip.reg_rows(pd, qd, dev(table), state, slots[1], face=dev(face), normals_in_source=in_source, work=work)
        assert np.array_equal(got, slots[1].cpu().numpy()), "a face list gives other bits than per-pair normals"


def test_rows_on_general_values():
    """General fp32 values under a general similarity: the terms are no longer exact, so the bound has a second part for their
    evaluation -- every term is a product of two factors of size at most g = 1 + |x - c| + |x - q| (unit normals), each a few
    dozen double roundings of coordinates of size at most ~8 g: 4096 x 2^-52 sum g^2 covers it with two orders to spare."""
    from multiply_amd import hip
    rng = np.random.RandomState(7)
    n = 4099
    st = RR.new_state(1.07, RS.rotation(AXIS, 21.0), [0.3, -0.2, 1.1], [-1, -1.2, 0.4], [1.3, 0.9, 2.2], tau2=0.04)
    p = rng.normal(0, 0.6, (n, 3)).astype(np.float32)
    u = rng.normal(0, 1, (n, 3))
    nrm = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    d = np.where(rng.uniform(0, 1, n) < 0.8, rng.uniform(0, 0.19, n), rng.uniform(0.21, 0.5, n))       # tau = 0.2
    v = rng.normal(0, 1, (n, 3))
    q = (RR.apply(st, p) + d[:, None] * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    want, want_mask, terms = RR.rows(p, q, nrm, st, True)
    assert np.abs(terms[want_mask == 0][:, RR.D2] / 0.04 - 1).min() > 1e-3
    x = RR.apply(st, p)
    g = 1 + np.linalg.norm(x - st[RR.C:RR.C + 3], axis=1) + np.linalg.norm(x - q, axis=1)
    slot = torch.zeros(hip.REG_SLOT, dtype=torch.float64, device="cuda")
    mask = torch.empty(n, dtype=torch.uint8, device="cuda")
    got = hip.reg_rows(dev(p), dev(q), dev(nrm), dev(st), slot, normals_in_source=True, mask=mask).cpu().numpy()
    assert np.array_equal(mask.cpu().numpy(), want_mask) and got[RR.N_ACC] == want[RR.N_ACC] and got[RR.N_REJ] == want[RR.N_REJ] > 0
    bound = n * EPS * np.abs(terms).sum(0) + 4096 * EPS * (g * g)[want_mask == 0].sum()
    print(f"[rows, general values] worst |sum - float64| / bound = {(np.abs(got - want)[:37] / bound[:37]).max():.3e}")
    assert (np.abs(got - want)[:37] <= bound[:37]).all()


# ------------------------------------------------------------------------------------------------ mp_reg_step
def test_step_against_the_reference_solve():
    """slots the test writes (two of them: the step adds them in order).  From s = 1, R = I, t = c = 0 the new state IS the update:
    t' = v, R' = exp([omega]x), s' = exp(sigma); each is compared with the reference's composition of numpy.linalg.solve's delta to
    within cond(A) 2^-52 |delta| -- the bound of the host program's test -- plus 8 roundings of the composition."""
    from multiply_amd import hip
    rng = np.random.RandomState(11)
    st0 = RR.new_state(1.0, np.eye(3), np.zeros(3), [-1, -1.5, -0.5], [1, 1.5, 0.5])
    worst = 0.0
    for k in range(24):
        B = rng.normal(0, 1, (12, 7))
        if k % 3 == 2:
            B = B @ np.diag(10.0 ** rng.uniform(-2, 2, 7))
        A, b = B.T @ B, (B.T @ B) @ np.append(rng.normal(0, 1e-2, 6), rng.normal(0, 1e-2))
        sums = RR.sums_from(A, b)
        half = sums * rng.uniform(0.2, 0.8, sums.shape)
        slots = np.stack([half, sums - half])
        similarity = k % 2
        state = dev(st0)
        hip.reg_step(dev(slots), state, similarity=similarity, reject=2.0, tol=0.0)
        got = state.cpu().numpy()
        m = 7 if similarity else 6
        total = slots[0] + slots[1]
        want, d = RR.step(total, st0, similarity, reject=2.0, tol=0.0)
        Am, bm = RR.normal_matrix(total, m)
        bound = np.linalg.cond(Am) * EPS * np.linalg.norm(d) + 8 * EPS
        err = np.abs(got[:13] - want[:13]).max()
        worst = max(worst, err / bound)
        assert got[RR.FLAG] == 0 and got[RR.ITERS] == 1 and err <= bound, (k, err, bound)
        assert got[RR.ACCEPTED] == 100 and abs(got[RR.RMS] - want[RR.RMS]) <= 2 * EPS * want[RR.RMS] and got[RR.TAU2] == (2.0 * got[RR.RMS]) ** 2
        assert abs(got[RR.STEP] - want[RR.STEP]) <= 4 * bound
    print(f"[step vs the reference] worst |state - reference| / (cond 2^-52 |delta| + 8 x 2^-52) = {worst:.3f}")
    st = st0.copy()
    state = dev(st)
    hip.reg_step(dev(np.stack([RR.sums_from(A, b)])), state, similarity=True, reject=0.0, tol=10.0)       # any step converges
    got = state.cpu().numpy()
    assert got[RR.FLAG] == RR.CONVERGED and np.isinf(got[RR.TAU2]) and got[RR.STEP] > 0


def _plane_pairs(n, rng, parallel):
    p = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    u = rng.normal(0, 1, (n, 3))
    nrm = np.tile([0.0, 0.0, 1.0], (n, 1)) if parallel else u / np.linalg.norm(u, axis=1, keepdims=True)
    q = (p + 0.01 * rng.normal(0, 1, (n, 3))).astype(np.float32)
    return dev(p), dev(q), dev(nrm.astype(np.float32))


def test_flagged_states_are_left_alone_and_degenerate_inputs_are_flagged():
    from multiply_amd import hip
    rng = np.random.RandomState(12)
    box = ([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5])
    slots = torch.zeros(1, hip.REG_SLOT, dtype=torch.float64, device="cuda")
    # a run that converges (a huge tol), then more rows + step launches: the state keeps its bits, the slot too
    state = dev(RR.new_state(1.0, np.eye(3), np.zeros(3), *box))
    p, q, nrm = _plane_pairs(300, rng, parallel=False)
    hip.reg_rows(p, q, nrm, state, slots[0])
    hip.reg_step(slots, state, similarity=True, tol=1.0)
    before, slot_before = state.cpu().numpy().copy(), slots.cpu().numpy().copy()
    assert before[RR.FLAG] == RR.CONVERGED and before[RR.ITERS] == 1
    p2, q2, n2 = _plane_pairs(500, rng, parallel=False)
    for _ in range(3):
        hip.reg_rows(p2, q2, n2, state, slots[0])
        hip.reg_step(slots, state, similarity=True, tol=1.0)
    assert np.array_equal(state.cpu().numpy(), before) and np.array_equal(slots.cpu().numpy(), slot_before)
    # fewer than 7 accepted pairs
    for n in (0, 6):
        state = dev(RR.new_state(1.0, np.eye(3), np.zeros(3), *box))
        p, q, nrm = _plane_pairs(n, rng, parallel=False)
        hip.reg_rows(p, q, nrm, state, slots[0])
        hip.reg_step(slots, state)
        got = state.cpu().numpy()
        assert got[RR.FLAG] == RR.DEGENERATE and got[RR.ACCEPTED] == n and np.array_equal(got[:13], RR.new_state(1.0, np.eye(3), np.zeros(3), *box)[:13])
    # all normals parallel: the plane's in-plane motions are free, the matrix has rank 3
    for similarity in (False, True):
        st0 = RR.new_state(1.1, RS.rotation(AXIS, 5), [0.01, 0.02, 0.03], *box)
        state = dev(st0)
        p, q, nrm = _plane_pairs(400, rng, parallel=True)
        hip.reg_rows(p, q, nrm, state, slots[0])
        hip.reg_step(slots, state, similarity=similarity)
        got = state.cpu().numpy()
        assert got[RR.FLAG] == RR.DEGENERATE and got[RR.ACCEPTED] == 400 and np.array_equal(got[:13], st0[:13]) and got[RR.ITERS] == 0
        hip.reg_step(slots, state, similarity=similarity)
        assert np.array_equal(state.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ mp_reg_fit_pairs
@pytest.mark.parametrize("similarity", [False, True])
@pytest.mark.parametrize("n", [3, 64, 6890])
def test_fit_pairs_against_the_reference(n, similarity):
    """Bounds as k_pose_errors states them for its Procrustes sums: the sums carry n 2^-53 relative (two passes about the means, no
    cancellation), the rotation 1e-12 / gap (gap = (S_2 + D_3 S_3) / S_1: how well the rotation is determined).  s is a quotient
    of two such sums (tr(S D) to 1e-14 S_1 by the routine's own test); t = q_ - s R p_ inherits both through |p_|."""
    from multiply_amd import hip
    rng = np.random.RandomState(20 + n)
    p = (rng.normal(0, 0.4, (n, 3)) * [1.0, 1.6, 0.7] + [0.2, -0.1, 2.5]).astype(np.float32)
    R0, t0, s0 = RS.rotation(AXIS, 33.0), np.array([0.1, 0.3, -0.2]), 1.3 if similarity else 1.0
    q = (s0 * p.astype(np.float64) @ R0.T + t0 + rng.normal(0, 0.01, (n, 3))).astype(np.float32)
    w = rng.uniform(0.1, 2.0, n).astype(np.float32)
    if n > 3:
        w[rng.uniform(0, 1, n) < 0.2] = 0.0
    out = hip.reg_fit_pairs(dev(p), dev(q), dev(w), similarity).cpu().numpy()
    again = hip.reg_fit_pairs(dev(p), dev(q), dev(w), similarity).cpu().numpy()
    assert np.array_equal(out, again)
    keep = w > 0
    s, Rm, t, Sg, D = RR.umeyama(p[keep], q[keep], w[keep], similarity)
    gs, gR, gt = out[0], out[1:10].reshape(3, 3), out[10:13]
    gap = (Sg[1] + D[2] * Sg[2]) / Sg[0]
    rel = n * 2.0 ** -53
    pm = np.abs((w[keep, None] * p[keep]).sum(0) / w[keep].sum()).max()
    e_s, e_R = abs(gs - s), np.abs(gR - Rm).max()
    b_s = (2 * rel + 1e-14) * s
    b_R = 1e-12 / gap
    b_t = rel * (np.abs(t).max() + 2 * s * pm) + pm * (b_s + s * b_R)
    print(f"[fit_pairs n={n} similarity={similarity}] gap {gap:.3f}; off: s {e_s:.2e} ({b_s:.2e})  R {e_R:.2e} ({b_R:.2e})  "
          f"t {np.abs(gt - t).max():.2e} ({b_t:.2e})  sum w {abs(out[13] - w.astype(np.float64).sum()):.2e}")
    assert out[15] == 0 and out[14] == (~keep).sum()
    assert abs(out[13] - w.astype(np.float64).sum()) <= rel * w.astype(np.float64).sum()
    assert (e_s <= b_s if similarity else gs == 1.0) and e_R <= b_R and np.abs(gt - t).max() <= b_t
    assert np.abs(gR @ gR.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(gR) - 1) <= 1e-14
    T = reg.fit_pairs(p, q, w, "similarity" if similarity else "rigid")
    assert T.scale == gs and np.array_equal(T.R, gR) and np.array_equal(T.t, gt)


def test_fit_pairs_leaves_out_what_it_cannot_use():
    from multiply_amd import hip
    rng = np.random.RandomState(30)
    p = rng.normal(0, 1, (40, 3)).astype(np.float32)
    q = (p.astype(np.float64) @ RS.rotation(AXIS, 70).T + [1, 2, 3]).astype(np.float32)
    clean = hip.reg_fit_pairs(dev(p[5:]), dev(q[5:]), None, True).cpu().numpy()
    p2, q2, w = p.copy(), q.copy(), np.ones(40, np.float32)
    p2[0, 1], q2[1, 2], w[2], w[3], w[4] = np.nan, np.inf, np.nan, -1.0, 0.0
    got = hip.reg_fit_pairs(dev(p2), dev(q2), dev(w), True).cpu().numpy()
    assert got[14] == 5 and got[13] == 35 and np.allclose(got[:13], clean[:13], rtol=0, atol=1e-13)
    none = hip.reg_fit_pairs(dev(p), dev(q), dev(np.zeros(40, np.float32)), True).cpu().numpy()
    assert none[15] == 1 and none[0] == 1 and np.array_equal(none[1:10].reshape(3, 3), np.eye(3))
    with pytest.raises(ValueError, match="no pair"):
        reg.fit_pairs(p, q, np.zeros(40, np.float32))


# ------------------------------------------------------------------------------------------------ the loop
@pytest.fixture(scope="module")
def shapes():
    v, f = RS.bumpy(3)
    v2, f2 = RS.bumpy(2)
    t0 = np.array([0.05, -0.04, 0.03])
    T0 = {"rigid": reg.Similarity(1.0, RS.rotation(AXIS, 25.0), t0), "similarity": reg.Similarity(0.9, RS.rotation(AXIS, 15.0), t0)}
    return dict(v=v, f=f, v2=v2, f2=f2, T0=T0, dst={k: RS.moved(v, T.R, T.t, T.scale) for k, T in T0.items()})


@pytest.mark.parametrize("kind", ["rigid", "similarity"])
def test_one_step_in_lockstep_with_the_reference(shapes, kind):
    """register with max_iters = 1; the reference redoes that step in float64 from the device's own samples, closest points, faces
    and accept masks.  The new code alone is under test here (the closest query has tests of its own)."""
    details = {}
    T, info = reg.register((shapes["v"], shapes["f"]), (shapes["dst"][kind], shapes["f"]), kind=kind, n_samples=2000, max_iters=1,
                           details=details)
    (it,) = details["iterations"]
    cpu = lambda t: t.cpu().numpy()
    total = np.zeros(RR.SLOT)
    for sl, dev_sums in zip(it["slots"], it["slot_sums"]):
        sums, _, _ = RR.rows(cpu(sl["p"]), cpu(sl["q"]), cpu(sl["normals"]), it["state_before"], sl["normals_in_source"], cpu(sl["face"]),
                             mask=cpu(sl["mask"]))
        assert (cpu(sl["mask"]) == 0).all() and sums[RR.N_ACC] == 2000 == dev_sums[RR.N_ACC]
        total += sums
    want, _ = RR.step(total, it["state_before"], kind == "similarity")
    got = it["state_after"]
    err = np.abs(got[:13] - want[:13]).max()
    print(f"[lockstep {kind}] |device - float64| over s, R, t: {err:.2e}; rms {got[RR.RMS]:.4f}, step {got[RR.STEP]:.4f}")
    assert err <= 1e-10 and info["iterations"] == 1 and not info["degenerate"]
    assert T.scale == got[RR.S] and np.array_equal(T.t, got[RR.T:RR.T + 3])


@pytest.fixture(scope="module")
def recovered(shapes):
    out = {}
    for kind in ("rigid", "similarity"):
        src, dst = (shapes["v"], shapes["f"]), (shapes["dst"][kind], shapes["f"])
        T, info = reg.register(src, dst, kind=kind, n_samples=2000, init="centroid", index_mode="brute")
        out[kind] = (T, info)
    return out


@pytest.mark.parametrize("kind", ["rigid", "similarity"])
def test_exact_copy_is_recovered_end_to_end(shapes, recovered, kind):
    T, info = recovered[kind]
    T0, v = shapes["T0"][kind], shapes["v"]
    bound = exact_copy_bound(v, shapes["dst"][kind])
    err = np.abs(T.apply(v) - T0.apply(v)).max()
    print(f"[exact copy {kind}] max_v |T v - T0 v| = {err:.3e} (bound {bound:.3e}); {info['iterations']} iterations, rms {info['rms']:.3e}, "
          f"rotation off {RS.rotation_angle_deg(T.R, T0.R):.2e} deg, scale off {abs(T.scale - T0.scale):.2e}; "
          f"accepted {info['accepted']} rejected {info['rejected']}")
    assert info["converged"] and not info["degenerate"] and info["left_out"] == 0
    assert err <= bound
    if kind == "rigid":
        assert T.scale == 1.0


@pytest.mark.parametrize("kind", ["rigid", "similarity"])
def test_brute_force_and_index_give_the_same_bits_and_runs_repeat(shapes, recovered, kind):
    src, dst = (shapes["v"], shapes["f"]), (shapes["dst"][kind], shapes["f"])
    states = []
    for mode in ("brute", "index", "index"):
        details = {}
        reg.register(src, dst, kind=kind, n_samples=2000, init="centroid", index_mode=mode, details=details)
        states.append(details["state"])
    assert np.array_equal(states[0], states[1]) and np.array_equal(states[1], states[2])
    T = recovered[kind][0]                 # the run without details, checked every 5 iterations: the same bits again
    assert T.scale == states[0][RR.S] and np.array_equal(T.R.reshape(9), states[0][RR.R:RR.R + 9]) and np.array_equal(T.t, states[0][RR.T:RR.T + 3])


@pytest.mark.parametrize("kind", ["rigid", "similarity"])
def test_different_tessellations(shapes, kind):
    """bumpy-320 onto the transformed bumpy-1280: no end state to compare (the iteration does not reach a fixed point); the
    symmetric surface RMS at the result, on fresh samples, is at most 1.01 x that at T0, and the rotation is within 1 degree.

    MEASURED on an MI355X with the defaults (seed 0, reject 3): rigid -- ratio 1.0005, 0.068 degrees, converged after 11 iterations;
    similarity -- ratio 0.6616, 0.137 degrees, converged after 12.  The samples are stratified over the area CDF
    (registration.sample_uniforms): with independent uniforms the rigid ratio was 1.0134 (0.52 degrees, no convergence in 30
    iterations), and the float64 reference on five sample sets gave 0.9999 .. 1.0124 against 0.9992 .. 1.0016 stratified (DESIGN
    6m)."""
    from multiply_amd import metrics
    T0 = shapes["T0"][kind]
    src, dst = (shapes["v2"], shapes["f2"]), (shapes["dst"][kind], shapes["f"])
    T, info = reg.register(src, dst, kind=kind, n_samples=600)
    rms = lambda A: (metrics.mesh_metrics((A.apply(shapes["v2"]).astype(np.float32), shapes["f2"]), dst, n_samples=4096, seed=99)["chamfer_sq"] / 2) ** 0.5
    at_T, at_T0, angle = rms(T), rms(T0), RS.rotation_angle_deg(T.R, T0.R)
    print(f"[tessellations {kind}] surface RMS at the result {at_T:.5e}, at T0 {at_T0:.5e} (ratio {at_T / at_T0:.4f}); rotation off {angle:.3f} deg; "
          f"{info['iterations']} iterations, converged {info['converged']}; step sizes at the read-backs "
          + " ".join(f"{h['step']:.1e}" for h in info["history"]))
    assert not info["degenerate"] and at_T <= 1.01 * at_T0 and angle <= 1.0


def test_register_sequence_recovers_the_shared_transform(shapes):
    """Three frames: frame k is bumpy-1280 under its own rigid motion M_k, the targets are those under ONE similarity S on top.
    register_sequence of the frames recovers S to the exact-copy bound; registering the unmoved shape onto each target alone
    returns S M_k, the frame's own motion, instead."""
    v, f = shapes["v"], shapes["f"]
    S = reg.Similarity(0.9, RS.rotation(AXIS, 15.0), [0.05, -0.04, 0.03])
    M = [reg.Similarity(1.0, RS.rotation(a, d), t) for a, d, t in (((0, 0, 1), 6.0, (0.02, 0.0, -0.01)), ((1, 0, 0), -8.0, (-0.03, 0.02, 0.0)),
                                                                     ((1, 1, 0), 5.0, (0.0, -0.02, 0.03)))]
    srcs = [RS.moved(v, m.R, m.t) for m in M]
    dsts = [RS.moved(sv, S.R, S.t, S.scale) for sv in srcs]
    T, info = reg.register_sequence([(sv, f) for sv in srcs], [(dv, f) for dv in dsts], kind="similarity", n_samples=2000)
    bound = exact_copy_bound(*srcs, *dsts)
    err = max(np.abs(T.apply(sv) - S.apply(sv)).max() for sv in srcs)
    print(f"[sequence] max_v |T v - S v| = {err:.3e} (bound {bound:.3e}); {info['iterations']} iterations, accepted {info['accepted']}")
    assert info["converged"] and info["n_frames"] == 3 and info["accepted"] + info["rejected"] == 3 * 2 * 2000 and err <= bound
    for k, m in enumerate(M):
        Tk, ik = reg.register((v, f), (dsts[k], f), kind="similarity", n_samples=2000)
        want = S.compose(m)
        ek = np.abs(Tk.apply(v) - want.apply(v)).max()
        print(f"[sequence, frame {k} alone] max_v |T_k v - S M_k v| = {ek:.3e}; |T_k v - S v| = {np.abs(Tk.apply(v) - S.apply(v)).max():.3e}")
        assert ik["converged"] and ek <= bound and np.abs(Tk.apply(v) - S.apply(v)).max() > 1000 * bound


# ------------------------------------------------------------------------------------------------ mesh_metrics(align=...)
@pytest.mark.parametrize("kind", ["rigid", "similarity"])
def test_mesh_metrics_aligns_a_moved_copy(shapes, kind):
    from multiply_amd import hip, metrics
    v, f = shapes["v"], shapes["f"]
    pred, gt = (shapes["dst"][kind], f), (v, f)
    out = metrics.mesh_metrics(pred, gt, n_samples=4096, iou_resolution=32, align=kind, align_options=dict(n_samples=2000))
    bound = exact_copy_bound(v, shapes["dst"][kind])
    assert set(out["align"]) == {"kind", "scale", "matrix", "rms", "iterations", "converged"} and out["align"]["converged"]
    T = reg.Similarity.from_matrix(out["align"]["matrix"])
    want = shapes["T0"][kind].inverse()
    aligned = reg.transform_vertices(dev(pred[0]), T).cpu().numpy()
    lo, hi = np.minimum(aligned.min(0), v.min(0)), np.maximum(aligned.max(0), v.max(0))
    centres = MR.lattice(lo, hi, 32)
    d2 = hip.mesh_closest(dev(centres), dev(v[f]))[0].cpu().numpy().astype(np.float64)
    inside = hip.mesh_signed_distance(dev(centres), dev(v[f])).cpu().numpy() < 0
    near = int((np.sqrt(d2) <= 2 * bound).sum())             # the bound, and as much again for the fp32 distance itself
    floor = 0.999 if near == 0 else 1.0 - near / max(int(inside.sum()), 1)
    print(f"[mesh_metrics align={kind}] chamfer {out['chamfer']:.3e} (bound {bound:.3e}), volume_iou {out['volume_iou']:.6f} (floor {floor:.6f}, "
          f"{near} lattice centres near the surface), |T - T0^-1| {np.abs(T.matrix - want.matrix).max():.2e}")
    assert out["chamfer"] <= bound and out["volume_iou"] >= floor
    given = metrics.mesh_metrics(pred, gt, n_samples=4096, align=T)
    assert given["align"]["kind"] == "given" and given["chamfer"] == out["chamfer"]


def test_mesh_metrics_without_align_is_what_it_was(shapes):
    from multiply_amd import metrics
    pred, gt = (shapes["dst"]["rigid"], shapes["f"]), (shapes["v"], shapes["f"])
    a = metrics.mesh_metrics(pred, gt, n_samples=4096, thresholds=(0.05, 0.1), seed=4, iou_resolution=12)
    b = metrics.mesh_metrics(pred, gt, n_samples=4096, thresholds=(0.05, 0.1), seed=4, iou_resolution=12, align=None)
    assert list(a) == list(b) and "align" not in a
    for k in a:
        assert np.array_equal(np.asarray(a[k], np.float64).view(np.int64), np.asarray(b[k], np.float64).view(np.int64)), k


# ------------------------------------------------------------------------------------------------ tools/eval_meshes.py
def test_eval_tool_aligns_two_folders_with_one_shared_transform(shapes, tmp_path, capsys):
    import importlib.util
    import json
    import os
    from multiply_amd.metrics import load_ply
    spec = importlib.util.spec_from_file_location("eval_meshes", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "tools", "eval_meshes.py"))
    E = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(E)
    v, f = shapes["v"], shapes["f"]
    S = shapes["T0"]["similarity"]
    pred, gt, out_dir = tmp_path / "pred", tmp_path / "gt", tmp_path / "aligned"
    pred.mkdir(), gt.mkdir()
    frames = {"0000.ply": RS.moved(v, RS.rotation((0, 0, 1), 6.0), (0.02, 0.0, -0.01)), "0001.ply": RS.moved(v, RS.rotation((1, 0, 0), -8.0), (-0.03, 0.02, 0.0))}
    for name, pv in frames.items():
        E.write_ply(str(pred / name), pv, f)
        E.write_ply(str(gt / name), RS.moved(pv, S.R, S.t, S.scale), f)
    E.write_ply(str(pred / "extra.ply"), v, f)
    res = E.main([str(pred), str(gt), "--samples", "2048", "--align", "similarity", "--align-shared", "--align-samples", "2000",
                  "--save-aligned", str(out_dir)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == json.loads(json.dumps(res))
    bound = exact_copy_bound(*frames.values(), *(RS.moved(pv, S.R, S.t, S.scale) for pv in frames.values()))
    assert sorted(res["frames"]) == sorted(frames) and res["unmatched"] == {"pred": ["extra.ply"], "gt": []}
    assert res["align"]["converged"] and np.abs(np.array(res["align"]["matrix"]) - S.matrix).max() <= bound
    for name, pv in frames.items():
        assert res["frames"][name]["chamfer"] <= bound and res["frames"][name]["align"]["kind"] == "given"
        av, af = load_ply(str(out_dir / name))
        assert np.array_equal(af, f) and np.abs(av - S.apply(pv)).max() <= bound
    assert res["mean"]["chamfer"] == sum(r["chamfer"] for r in res["frames"].values()) / 2
    one = E.main([str(pred / "0000.ply"), str(gt / "0000.ply"), "--samples", "2048", "--align", "similarity", "--align-samples", "2000"])
    assert one["align"]["kind"] == "similarity" and one["chamfer"] <= bound
