"""mp_kp_objective / mp_kp_fit and multiply_amd.keypoint_fit on the device against the float64 restatement
(tests/keypoint_fit_reference.py; inputs and float64 results: tests/keypoint_fit_cases.py, computed once per process).  Every
figure is printed before it is asserted; the bounds and what was measured: tests/tolerances_keypoint_fit.py."""
import numpy as np
import pytest
import torch

from multiply_amd import keypoint_fit as KF
from tests import keypoint_fit_cases as C
from tests import tolerances_keypoint_fit as TOL

pytestmark = pytest.mark.gpu
GROUPS = (("transl", slice(0, 3)), ("thetas", slice(3, 75)), ("betas", slice(75, 85)))


@pytest.fixture(scope="module")
def server(smpl_tables):
    from multiply_amd.smpl import SMPLServer
    return SMPLServer(smpl_tables=smpl_tables)


@pytest.fixture(scope="module")
def packs(server):
    return {name: m.pack(server) for name, m in C.maps().items()}


def _f32(x):
    return x.float().cuda()


def _objective(server, packs, name, rows, **kw):
    cs, _ = C.objective_reference(name)
    sel = list(rows)
    return KF.keypoint_objective(server, _f32(cs["params"][sel]), _f32(cs["targets"][sel]), None, cs["kmap"], _f32(cs["cam"][sel]),
                                 prev=_f32(cs["prev"][sel]), c=_f32(cs["c"][sel]), pack=packs[name], **kw)


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("rows", [(2,), (0, 1, 2)], ids=["N1", "N3"])
@pytest.mark.parametrize("name", ["joints", "vertices", "mixed", "coco25-shaped"])
def test_objective_against_float64(server, packs, name, rows):
    cs, ref = C.objective_reference(name)
    assert (cs["c"] == 0).any() and (cs["c"] > 0).any()
    res = (cs["targets"] - torch.stack([r[2] for r in ref])).abs()
    assert (res > 300).any() and (res < 20).any()                   # residuals well above and well below rho = 100
    out = _objective(server, packs, name, rows)
    assert not out["flags"].any()
    worst = dict(terms=0.0, proj=0.0, transl=0.0, thetas=0.0, betas=0.0)
    for i, n in enumerate(rows):
        terms, grad, proj, _ = ref[n]
        worst["terms"] = max(worst["terms"], float(((out["terms"][i].cpu().double() - terms).abs() / terms.abs()).max()))
        worst["proj"] = max(worst["proj"], float((out["proj"][i].cpu().double() - proj).abs().max()))
        for g, sl in GROUPS:
            worst[g] = max(worst[g], _rel(out["grad"][i].cpu().double()[sl], grad[sl]))
    print(f"objective {name} rows {rows}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["terms"] <= TOL.OBJ_TERMS_REL and worst["proj"] <= TOL.OBJ_PROJ_PX
    for g, _ in GROUPS:
        assert worst[g] <= TOL.OBJ_GRAD_REL[g], g


def _fit(server, packs, name, rows, iters, history=True, **kw):
    cs, _ = C.objective_reference(name)
    sel = list(rows)
    return KF.refine_frame(server, _f32(cs["params"][sel]), _f32(cs["targets"][sel]), _f32(cs["c"][sel]), _f32(cs["cam"][sel]),
                           cs["kmap"], prev=_f32(cs["prev"][sel]), iters=iters, lr=1e-3, history=history, pack=packs[name], **kw)


def _fit_errors(out, ref, rows, iters):
    ep = eh = 0.0
    for i, n in enumerate(rows):
        snap, hist = ref[n]
        ep = max(ep, float((out["params"][i].cpu().double() - snap[iters]).abs().max()))
        if iters:
            h = hist[:iters]
            eh = max(eh, float(((out["history"][i].cpu().double() - h).abs() / h.abs()).max()))
    return ep, eh


@pytest.mark.parametrize("rows", [(1,), (0, 1, 2)], ids=["N1", "N3"])
@pytest.mark.parametrize("iters", C.FIT_ITERS)
def test_fit_against_the_float64_loop(server, packs, iters, rows):
    cs, ref = C.fit_reference("mixed")
    out = _fit(server, packs, "mixed", rows, iters)
    assert tuple(out["history"].shape) == (len(rows), iters, 3) and not out["flags"].any()
    if iters == 0:
        assert torch.equal(out["params"].cpu(), cs["params"][list(rows)].float())         # a copy
        return
    ep, eh = _fit_errors(out, ref, rows, iters)
    print(f"fit iters {iters} rows {rows}: params {ep:.3e}, history {eh:.3e}")
    assert ep <= TOL.FIT_PARAMS_ABS[iters] and eh <= TOL.FIT_HISTORY_REL[iters]


@pytest.mark.parametrize("which", ["2d", "temporal"])
def test_each_term_alone(server, packs, which):
    w = dict(w_t=0.0) if which == "2d" else dict(w_2d=0.0)
    ref_w = dict(w_2d=C.R.REF["w_2d"], w_t=0.0) if which == "2d" else dict(w_2d=0.0, w_t=C.R.REF["w_t"])
    _, ref = C.fit_reference("mixed", 25, **ref_w)
    rows = (0, 1, 2)
    out = _fit(server, packs, "mixed", rows, 25, **w)
    ep = eh = 0.0
    for i, n in enumerate(rows):
        snap, hist = ref[n]
        ep = max(ep, float((out["params"][i].cpu().double() - snap[25]).abs().max()))
        # the term that is switched off is still reported; the total is the other one alone
        eh = max(eh, float(((out["history"][i].cpu().double() - hist).abs() / hist.abs().clamp_min(1e-30)).max()))
        k = 0 if which == "2d" else 1
        wk = ref_w["w_2d"] if which == "2d" else ref_w["w_t"]
        assert torch.equal(out["history"][i, :, 2], (out["history"][i, :, k] * np.float32(wk) + 0.0))
    print(f"fit, {which} term alone: params {ep:.3e}, history {eh:.3e}")
    assert ep <= TOL.FIT_ONE_TERM_PARAMS_ABS[which] and eh <= TOL.FIT_ONE_TERM_HISTORY_REL[which]


def test_one_step_is_adam_on_the_objectives_gradient_bit_for_bit(server, packs):
    cs, _ = C.objective_reference("coco25-shaped")
    rows = (0, 1, 2)
    g = _objective(server, packs, "coco25-shaped", rows)["grad"]
    out = _fit(server, packs, "coco25-shaped", rows, 1)
    p = _f32(cs["params"])
    f = lambda x: torch.full_like(g, float(x))
    b1, b2, lr = np.float32(0.9), np.float32(0.999), np.float32(1e-3)
    m = g * f(np.float32(1) - b1)
    v = (f(np.float32(1) - b2) * g) * g
    step = np.float32(float(lr) / (1.0 - float(b1)))
    denom = v.sqrt() / f(np.float32(np.sqrt(1.0 - float(b2)))) + f(np.float32(1e-8))
    want = (p.double() - float(step) * (m / denom).double()).float()      # the kernel's fmaf(-step, m / denom, p)
    assert torch.equal(out["params"], want)
    assert torch.equal(out["history"][:, 0], _objective(server, packs, "coco25-shaped", rows)["terms"])


def test_same_bits_on_every_call_and_at_every_place_in_a_batch(server, packs):
    for name in ("mixed", "coco25-shaped"):
        a, b = _fit(server, packs, name, (0, 1, 2), 25), _fit(server, packs, name, (0, 1, 2), 25)
        assert torch.equal(a["params"], b["params"]) and torch.equal(a["history"], b["history"])
        alone = _fit(server, packs, name, (1,), 25)
        oa = _objective(server, packs, name, (1,))
        for rows in ((1, 0, 2), (0, 1, 2), (2, 0, 1)):                   # first, middle, last
            i = rows.index(1)
            batch = _fit(server, packs, name, rows, 25)
            assert torch.equal(batch["params"][i], alone["params"][0]) and torch.equal(batch["history"][i], alone["history"][0])
            ob = _objective(server, packs, name, rows)
            for k in ("terms", "grad", "proj"):
                assert torch.equal(ob[k][i], oa[k][0]), (name, rows, k)


def test_refine_sequence_recovers_like_the_float64_loop(server):
    cs, ref = C.recovery_case(), C.recovery_reference()
    init = dict(zip(("pose", "trans", "shape"), KF.split_params(cs["init"])))
    out = KF.refine_sequence([server, server], init, cs["keypoints"], dict(zip(("fx", "fy", "cx", "cy"), cs["cam"][:4].tolist())),
                             cs["kmap"], iters=C.REC_ITERS, tracking=C.REC_TRACKING, interpolate_frames=C.REC_INTERP)
    res = KF.pack_params(out["pose"], out["trans"], out["shape"]).cpu()
    assert tuple(res.shape) == (C.REC_F, C.REC_P, 85) and tuple(out["terms"].shape) == (C.REC_F, C.REC_P, 3) and not out["flags"].any()
    after = C.reprojection_error(cs, res)
    dp = float((res.double() - ref["results"]).abs().max())
    print(f"recovery: {ref['before']:.4f} px -> kernel {after:.4f} px, float64 loop {ref['after']:.4f} px (apart {abs(after - ref['after']):.3e} px); "
          f"params differ by {dp:.3e}")
    assert after <= 0.5 * ref["before"] and abs(after - ref["after"]) <= TOL.RECOVERY_PX
    assert torch.isfinite(out["terms"]).all()
    # frame f's temporal target is frame f - 1's output, bit for bit; frame 0's is its own start; the copied frame; the tracked start
    assert torch.equal(out["prev"][1:].cpu(), res[:-1, :, :75]) and torch.equal(out["prev"][0].cpu(), cs["init"][0][:, :75])
    assert torch.equal(res[1][:, :75], res[0][:, :75]) and torch.equal(res[1][:, 75:], cs["init"][1][:, 75:])
    kmap = cs["kmap"]
    kp = cs["keypoints"]
    start = cs["init"][2].clone()
    start[1] = res[1][1]
    again = KF.refine_frame([server, server], start, kp[2, :, :, :2], KF.keypoint_weights(kp[2, :, :, 2], kmap, 0.6),
                            dict(zip(("fx", "fy", "cx", "cy"), cs["cam"][:4].tolist())), kmap, prev=res[1][:, :75], iters=C.REC_ITERS)
    assert torch.equal(again["params"].cpu(), res[2])


def test_rejected_inputs(server, packs):
    from multiply_amd import hip
    cs, _ = C.objective_reference("mixed")
    pack = packs["mixed"]
    p = _f32(cs["params"]).clone()
    p[1, 2] = -3.0                                                     # row 1 stands behind the camera
    args = (p, _f32(cs["targets"]), None, cs["kmap"], _f32(cs["cam"]))
    out = KF.keypoint_objective(server, *args, prev=_f32(cs["prev"]), c=_f32(cs["c"]), pack=pack)
    assert out["flags"].tolist() == [0, 1, 0]
    assert float(out["terms"][1, 0]) == 0.0 and (out["proj"][1] == 0).all()
    for k in ("terms", "grad", "proj"):
        assert torch.isfinite(out[k]).all(), k
    fit = KF.refine_frame(server, p, _f32(cs["targets"]), _f32(cs["c"]), _f32(cs["cam"]), cs["kmap"], prev=_f32(cs["prev"]), iters=3,
                          pack=pack, history=True)
    assert fit["flags"].tolist() == [0, 1, 0] and torch.isfinite(fit["params"]).all() and torch.isfinite(fit["history"]).all()
    # sizes above the caps: status -2 without a launch (the module's own check comes first: KeypointMap raises ValueError)
    z = torch.zeros(4, dtype=torch.int32, device="cuda")
    for S, K in ((KF.MAX_S + 1, 1), (0, KF.MAX_K + 1), (0, 0)):
        t = list(pack.table_args(None))
        t[-2:] = [S, K]
        with pytest.raises(RuntimeError, match="mp_kp_objective failed with code -2"):
            hip.lib().mp_kp_objective(*t, p, None, _f32(cs["targets"]), _f32(cs["c"]), _f32(cs["cam"]), 3, 100.0, 1e-2, 6.0, 5.0,
                                      out["terms"], None, None, z, hip.stream())
        with pytest.raises(RuntimeError, match="mp_kp_fit failed with code -2"):
            hip.lib().mp_kp_fit(*t, p, None, _f32(cs["targets"]), _f32(cs["c"]), _f32(cs["cam"]), 3, 100.0, 1e-2, 6.0, 5.0, 1, 1e-3,
                                1e-3, 1e-3, 0.9, 0.999, 1e-8, out["grad"], None, z, hip.stream())
    with pytest.raises(ValueError, match=r"\(3, 84\)"):
        KF.keypoint_objective(server, p[:, :84], *args[1:], c=_f32(cs["c"]), pack=pack)
    with pytest.raises(ValueError, match="int64"):
        KF.keypoint_objective(server, p.long(), *args[1:], c=_f32(cs["c"]), pack=pack)
    proj, flags = KF.project_keypoints(server, _f32(cs["params"]), cs["kmap"], _f32(cs["cam"]), pack=pack)
    assert torch.equal(proj, _objective(server, packs, "mixed", (0, 1, 2))["proj"]) and not flags.any()
