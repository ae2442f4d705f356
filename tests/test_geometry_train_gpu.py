"""Differentiable volume depths on the device: mp_tr_composite_geometry_bwd through the C ABI against float64 autograd, and
Multiply.train_geometry end to end (forward keys, gradients against the oracle, mesh_losses.ray_depth_order_loss,
opt_depth_frame(depth_source='volume'), the refusal under person sharding).

The reference of the kernel is tests/geometry_train_reference.py (float64 torch autograd of a sort-based restatement of the five
differentiable outputs); the bounds are tests/tolerances_geometry_train.py.  On (ray, person) entries that
geometry_reference.exempt marks a float32 implementation may cross one sample off: the level upstream is 0 there, and at most
5 % of a case's crossing entries may be exempt."""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import geometry_train_reference as GT
from tests import tolerances_geometry_train as TOL

pytestmark = pytest.mark.gpu

GUARD_ROWS, TAIL = 2, 37          # table rows no ray refers to; floats past R_p * S (the eikonal tail of a dsdf_rows vector)
MEASURED = {}                     # running maxima, printed by every test that measures


def _note(name, value):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(value))


def _report():
    print("[geometry train] measured maxima so far:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


@functools.lru_cache(maxsize=None)
def reference(shape, beta, level, only):
    """float64 autograd of the case (all five upstream gradients, or the one named `only`) -> inv, z, sdf, up, d_sdf, d_beta, ref"""
    inv, z, sdf, ref, up = GT.case(shape, beta, level)
    if only is not None:
        up = {k: (v if k == only else None) for k, v in up.items()}
    d_sdf, d_beta = GT.autograd_gradients(shape[0], inv, z, sdf, float(np.float32(beta)), level, up)
    return inv, z, sdf, up, d_sdf, d_beta, ref


def launch(n_rays, inv, z, sdf, beta, level, up, scale=1.0, seed=0):
    """the entry point on numpy inputs.  Every person's tables get GUARD_ROWS rows that no ray refers to and d_sdf[p] a tail of
    TAIL floats; d_sdf and d_beta start from a seeded pattern of magnitude `scale`.
    -> (d_sdf after, d_sdf before, d_beta after, d_beta before) as numpy"""
    from multiply_amd import hip
    L = hip.lib()
    P, NZ = len(inv), z[0].shape[1]
    rs = np.random.RandomState(seed)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pad = lambda a: np.concatenate([a, np.repeat(a[-1:], GUARD_ROWS, 0)], 0)
    keep = [[dev(a) for a in inv], [dev(pad(a)) for a in z], [dev(pad(a)) for a in sdf]]
    tabs = [hip.device_ints([t.data_ptr() for t in ts], "cuda") for ts in keep]
    before = [(rs.randn((s.shape[0] + GUARD_ROWS) * s.shape[1] + TAIL) * scale).astype(np.float32) for s in sdf]
    d_sdf = [dev(b.copy()) for b in before]
    t_dsdf = hip.device_ints([t.data_ptr() for t in d_sdf], "cuda")
    beta_d = torch.tensor([beta], dtype=torch.float32, device="cuda")
    b0 = np.float32(rs.randn() * scale)
    d_beta = torch.tensor([b0], dtype=torch.float32, device="cuda")
    ups = [None if up.get(k) is None else dev(np.asarray(up[k], dtype=np.float32)) for k in GT.DIFF_KEYS]
    status = L.mp_tr_composite_geometry_bwd(n_rays, P, NZ, *tabs, beta_d, level, *ups, t_dsdf, d_beta, hip.stream())
    torch.cuda.synchronize()
    assert status == 0
    return [t.cpu().numpy() for t in d_sdf], before, float(d_beta.cpu()[0]), float(b0)


def check(tag, shape, beta, level, only=None):
    """launch the case, compare `result - pattern` with the reference, and the rows that must not change bit for bit"""
    inv, z, sdf, up, r_sdf, r_beta, ref = reference(shape, beta, level, only)
    # the scales are the CASE's (all five terms): one term alone can cancel to nothing in float64 -- the opacity of a saturated
    # person does not depend on its samples -- and is then no scale for a float32 error
    full = reference(shape, beta, level, None)
    top = max(float(np.abs(a).max()) for a in full[4])
    assert top > 0 and np.isfinite(top)
    got, before, gb, b0 = launch(shape[0], inv, z, sdf, beta, level, up, scale=0.25 * top)
    e_sdf = 0.0
    for n, (a, b, want) in enumerate(zip(got, before, r_sdf)):
        rows, S = sdf[n].shape
        used = np.zeros(rows + GUARD_ROWS, bool)
        used[np.asarray(inv[n])[np.asarray(inv[n]) >= 0]] = True
        a2, b2 = a[:(rows + GUARD_ROWS) * S].reshape(-1, S), b[:(rows + GUARD_ROWS) * S].reshape(-1, S)
        assert np.isfinite(a).all(), (tag, n)
        # table rows no ray of this launch refers to (guard rows, the one row of a person nobody hits) and the tail: bit-unchanged
        assert np.array_equal(a2[~used], b2[~used]), (tag, n)
        assert np.array_equal(a[(rows + GUARD_ROWS) * S:], b[(rows + GUARD_ROWS) * S:]), (tag, n)
        if used.any():
            e_sdf = max(e_sdf, float(np.abs((a2[:rows].astype(np.float64) - b2[:rows])[used[:rows]] - want[used[:rows]]).max()))
    e_beta = abs((gb - b0) - r_beta) / abs(full[5])
    _note("d sdf |err| / max |d sdf|", e_sdf / top)
    _note("d beta rel err", e_beta)
    print(f"[geometry train] {tag} {shape} beta {beta} level {level} only {only}: d sdf {e_sdf / top:.3e} of max {top:.3e}, "
          f"d beta {e_beta:.3e} of {r_beta:.3e}")
    return e_sdf / top, e_beta


# ------------------------------------------------------------------------------------------------ 4. kernel vs float64 autograd
@pytest.mark.parametrize("shape,beta,level", GT.CASES)
def test_kernel_against_float64_autograd(shape, beta, level):
    inv, z, sdf, up, _, _, ref = reference(shape, beta, level, None)
    hit = np.stack([np.asarray(iv) >= 0 for iv in inv], 1)
    cross = ref["depth_solo_level"] >= 0
    assert (cross == hit).all(), "every hit entry crosses"
    ex = G.exempt(ref["fe_cross_solo"], ref["margin_solo"]) & cross
    print(f"[geometry train] {shape} beta {beta} level {level}: {int(ex.sum())} of {int(cross.sum())} crossing entries exempt")
    assert ex.sum() <= 0.05 * cross.sum()
    assert (up["depth_solo_level"][ex] == 0).all() and (up["depth_solo_level"][cross & ~ex] != 0).all()
    e_sdf, e_beta = check("all", shape, beta, level)
    _report()
    assert e_sdf <= TOL.DSDF and e_beta <= TOL.DBETA, (e_sdf, e_beta)


@pytest.mark.parametrize("shape,beta,level", [GT.CASES[0], GT.CASES[4]])
def test_every_upstream_pointer_alone_and_none_at_all(shape, beta, level):
    for only in GT.DIFF_KEYS:
        e_sdf, e_beta = check("one", shape, beta, level, only)
        assert e_sdf <= TOL.DSDF and e_beta <= TOL.DBETA, (only, e_sdf, e_beta)
    _report()
    inv, z, sdf, up, _, _, _ = reference(shape, beta, level, None)
    got, before, gb, b0 = launch(shape[0], inv, z, sdf, beta, level, {})          # all NULL: status 0, nothing written
    assert all(np.array_equal(a, b) for a, b in zip(got, before)) and gb == b0


def test_fewer_rays_than_the_tables_hold():
    """n_rays = R - 3: the rows only the last three rays refer to stay bit-unchanged, the others are those of the full launch"""
    shape, beta, level = GT.CASES[0]
    inv, z, sdf, up, _, _, _ = reference(shape, beta, level, None)
    R = shape[0]
    full, before, _, _ = launch(R, inv, z, sdf, beta, level, up, seed=3)
    few, before2, _, _ = launch(R - 3, inv, z, sdf, beta, level, up, seed=3)
    assert all(np.array_equal(a, b) for a, b in zip(before, before2))
    # (RAGGED_HITS: rays 65..69 are hit by nobody, so take the last rays that are)
    for n in range(len(inv)):
        S = sdf[n].shape[1]
        iv = np.asarray(inv[n])
        a, b, c = (x[:sdf[n].shape[0] * S].reshape(-1, S) for x in (full[n], few[n], before[n]))
        late, early = iv[R - 3:][iv[R - 3:] >= 0], iv[:R - 3][iv[:R - 3] >= 0]
        assert np.array_equal(b[late], c[late]) and np.array_equal(b[early], a[early])
    few, before2, _, _ = launch(40, inv, z, sdf, beta, level, up, seed=3)
    iv = np.asarray(inv[1])
    S = sdf[1].shape[1]
    late = iv[40:][iv[40:] >= 0]
    assert len(late) and np.array_equal(few[1][:sdf[1].shape[0] * S].reshape(-1, S)[late], before[1][:sdf[1].shape[0] * S].reshape(-1, S)[late])


def test_argument_errors_make_no_launch():
    up = lambda R, P: dict(depth=np.ones(R, np.float32), depth_solo_level=np.ones((R, P), np.float32))
    inv, z, sdf = G.ragged_case(5, 9, 34, seed=1)
    with pytest.raises(RuntimeError, match="mp_tr_composite_geometry_bwd failed with code -1"):
        launch(5, inv, z, sdf, 0.02, 0.5, up(5, 9))
    inv, z, sdf = G.ragged_case(5, 2, 34, seed=1)
    for bad in (1.0, 0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="mp_tr_composite_geometry_bwd failed with code -3"):
            launch(5, inv, z, sdf, 0.02, bad, up(5, 2))
    inv, z, sdf = G.ragged_case(2, 8, 3000, seed=1)                               # one wave x 8 persons x 5 x 2999 floats of LDS
    with pytest.raises(RuntimeError, match="mp_tr_composite_geometry_bwd failed with code -2"):
        launch(2, inv, z, sdf, 0.02, 0.5, up(2, 8))
    got, before, gb, b0 = launch(0, inv[:1], z[:1], sdf[:1], 0.02, 0.5, up(2, 1))  # n_rays = 0: status 0, nothing written
    assert np.array_equal(got[0], before[0]) and gb == b0


# ------------------------------------------------------------------------------------------------ 5. the training step
GEO_KEYS = ("depth_values", "depth_person_list", "depth_level_values", "front_person", "acc_person_solo_list",
            "depth_person_solo_list", "depth_person_solo_level_list")
# the differentiable keys, in the order of geometry_train_reference.DIFF_KEYS
DIFF = dict(depth="depth_values", depth_person="depth_person_list", acc_solo="acc_person_solo_list",
            depth_solo="depth_person_solo_list", depth_solo_level="depth_person_solo_level_list")
BODY = ("smpl_pose", "smpl_trans", "smpl_shape")
EPOCH = 301


def hip_lib():
    from multiply_amd import hip
    return hip.lib()


def _labels(D):
    """(R,2) SAM logits naming, on the rays where both persons cross, the one whose solo level depth is LARGER (the order term is
    then active there); person 0 elsewhere"""
    both = (D >= 0).all(1)
    lab = torch.where(both & (D[:, 1] > D[:, 0]), 1, 0)
    logits = torch.full(tuple(D.shape), -12.0)
    logits[torch.arange(D.shape[0]), lab] = 12.0
    return logits, both


@functools.lru_cache(maxsize=None)
def _step():
    """11 x 11 rays, 2 persons, all rays hit, the body inputs under optimisation, ONE set of draws: the flag-off step before the
    attribute is ever set and after, the flag-on steps (the seeded geometry loss, the colour loss, both, the ray depth-order
    term), and the oracle under torch autograd on the device's depths -- computed once for the tests below."""
    from multiply_amd import mesh_losses as ML
    from multiply_amd import train as T
    from tests.test_train_step_gpu import _cpu, _train_setup
    model, oracle, inp, gin, gt, loss_fn, _ = _train_setup()
    assert "train_geometry" not in vars(model) and model.train_geometry is False
    R = inp["uv"].shape[1]
    hit = [torch.arange(R), torch.arange(R)]
    for k in BODY:
        gin[k] = gin[k].clone().requires_grad_(True)
    gin["smpl_pose_last"] = gin["smpl_pose"].detach() + 0.01
    cx = model._setup({**gin, "hit_index": hit}, -1, False)
    draws = T.make_draws(model, cx, None)
    res = dict(model=model, inp=inp, gin=gin, hit=hit, gt=gt, loss_fn=loss_fn, R=R)
    # every launch of the two geometry entry points is counted: with the flag off there must be none
    lib, calls = hip_lib(), {"mp_composite_geometry": 0, "mp_tr_composite_geometry_bwd": 0}
    real = {k: getattr(lib, k) for k in calls}

    def counting(name):
        def call(*a):
            calls[name] += 1
            return real[name](*a)
        return call
    for k in calls:
        setattr(lib, k, counting(k))

    def run(loss_of):
        out = T.forward_train(model, {**gin, "hit_index": hit}, draws=draws)
        loss = loss_of(out)
        model.zero_grad()
        for k in BODY:
            gin[k].grad = None
        loss.backward()
        torch.cuda.synchronize()
        return (out, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: gin[k].grad.detach().cpu().clone() for k in BODY})

    colour = lambda out: loss_fn(out, gt)["loss"]
    T.forward_train(model, {**gin, "hit_index": hit}, draws=draws)
    for p in range(2):                                   # every step on the depths of this first forward: one sampler run
        draws["person"][p]["z_given"] = model._last_train.fg[p]["zfinal"].clone()
    res["off_before"] = run(colour)
    res["off_again"] = run(colour)
    res["calls_off"] = dict(calls)
    model.train_geometry = True

    def geo_loss(out):
        return sum((res["g"][k].cuda() * out[DIFF[k]]).sum() for k in GT.DIFF_KEYS)

    # the seeded upstream gradients need the reference's exempt entries: a first flag-on forward gives the graph's own tables
    out = T.forward_train(model, {**gin, "hit_index": hit}, draws=draws)
    graph = model._last_train
    tabs = [[rec[k].detach().cpu().numpy() for rec in graph.composited] for k in ("inv", "z", "sdf")]
    NZ = tabs[1][0].shape[-1]
    tabs[1] = [a.reshape(-1, NZ) for a in tabs[1]]
    tabs[2] = [a.reshape(-1, NZ - 1)[:z.shape[0]] for a, z in zip(tabs[2], tabs[1])]
    beta = float(cx["beta"].reshape(-1)[0])
    res["ref"] = ref = G.geometry_reference(R, *tabs, beta, model.geometry_level)
    res["forward"] = {k: v.detach().cpu() for k, v in out.items() if k in GEO_KEYS}
    res["keys_on"] = set(out.keys())
    rs = np.random.RandomState(7)
    g = dict(depth=rs.randn(R), depth_person=rs.randn(R, 2), acc_solo=rs.randn(R, 2), depth_solo=rs.randn(R, 2),
             depth_solo_level=rs.randn(R, 2))
    g["depth_solo_level"][G.exempt(ref["fe_cross_solo"], ref["margin_solo"])] = 0.0
    res["g"] = {k: torch.from_numpy(v).float() for k, v in g.items()}
    res["on_geo"] = run(geo_loss)
    res["on_colour"] = run(colour)
    res["on_both"] = run(lambda out: colour(out) + geo_loss(out))
    res["calls_on"] = dict(calls)
    model.train_geometry = False
    res["off_after"] = run(colour)
    res["calls_off_after"] = dict(calls)
    model.train_geometry = True

    # the oracle on the device's depths and draws: per-person sdf with autograd -> the restatement's outputs
    for v in oracle.sd.values():
        if v.is_floating_point():
            v.requires_grad_(True)
    oin = dict(inp)
    for k in BODY:
        oin[k] = inp[k].clone().requires_grad_(True)
    z_given = [graph.fg[p]["zfinal"].cpu() for p in range(2)]
    want = oracle.forward_train(oin, hit, z_given, _cpu(draws))
    o_out = GT.geometry_outputs(R, [np.arange(R)] * 2, [z.double() for z in z_given], [s.double() for s in want["sdf"]],
                                oracle.beta().double(), model.geometry_level)
    res["oracle_forward"] = {k: v.detach() for k, v in o_out.items()}
    names = [k for k, v in oracle.sd.items() if v.requires_grad]
    o_loss = sum((res["g"][k].double() * o_out[k]).sum() for k in GT.DIFF_KEYS)
    gw = torch.autograd.grad(o_loss, [oracle.sd[k] for k in names] + [oin[k] for k in BODY], allow_unused=True, retain_graph=True)
    res["oracle_params"] = dict(zip(names, gw[:len(names)]))
    res["oracle_body"] = dict(zip(BODY, gw[len(names):]))
    # one ray depth-order step, labels from the oracle's depths
    logits, both = _labels(o_out["depth_solo_level"].detach())
    res["labels"], res["both"] = logits, both
    o_order = ML.ray_depth_order_loss({"depth_person_solo_level_list": o_out["depth_solo_level"]}, EPOCH, sam_mask=logits.double())
    res["oracle_order"] = (float(o_order), dict(zip(BODY, torch.autograd.grad(o_order, [oin[k] for k in BODY], allow_unused=True))))
    order = {}
    res["on_order"] = run(lambda out: order.setdefault("loss", ML.ray_depth_order_loss(out, EPOCH, sam_mask=logits.cuda())))
    res["order_loss"] = float(order["loss"])
    for k in calls:
        setattr(lib, k, real[k])
    return res


def _spread(pa, pb):
    """worst per-tensor relative L2 difference of two sets of parameter gradients; tensors within 1e-7 absolute count as equal"""
    worst = 0.0
    for k in pa:
        d = (pa[k] - pb[k]).double()
        if float(d.abs().max()) >= 1e-7:
            worst = max(worst, float(d.norm() / (pb[k].double().norm() + 1e-12)))
    return worst


def test_flag_off_is_the_step_of_before():
    """With the flag off the dict has today's keys, rgb_values is bit-identical to a run made before the attribute was ever set,
    and neither geometry entry point is launched.  The parameter gradients cannot be compared bit for bit: the weight gradients
    are fp32 atomic sums (mp_gemm_tn*), and two runs of the UNCHANGED step made before the attribute was ever set already differ
    bitwise in 112 of 112 tensors on the MI355X (by less than 1e-7 absolute in every tensor).  They are held to 1e-5 relative L2
    per tensor or 1e-7 absolute, the bound test_geometry_and_colour_losses_add_up uses for the same atomic-order noise (the two
    untouched runs' spread is printed; measured: no tensor beyond 1e-7 absolute, before or after the attribute was set)."""
    s = _step()
    out0, p0, _ = s["off_before"]
    assert len(out0) == 20 and not (set(GEO_KEYS) & set(out0.keys()))
    assert all(v == 0 for v in s["calls_off"].values()), s["calls_off"]
    assert s["calls_on"]["mp_composite_geometry"] > 0 and s["calls_on"]["mp_tr_composite_geometry_bwd"] > 0
    assert s["calls_off_after"] == s["calls_on"]                                     # flag off again: no further launch
    for name in ("off_again", "off_after"):
        out1, p1, _ = s[name]
        assert set(out1.keys()) == set(out0.keys()), name
        for k in ("rgb_values", "normal_values", "acc_map", "acc_person_list", "grad_theta"):
            assert torch.equal(out1[k], out0[k]), (name, k)
        assert p1.keys() == p0.keys()
        diff = [k for k in p0 if not torch.equal(p0[k], p1[k])]
        print(f"[geometry train] flag off, {name}: {len(diff)} of {len(p0)} parameter gradients differ bitwise from the first run; "
              f"worst relative L2 difference {_spread(p1, p0):.3e}")
    assert _spread(s["off_after"][1], p0) < 1e-5


def test_flag_on_forward_against_the_float64_reference():
    from tests import tolerances_geometry as TG
    s = _step()
    ref, got = s["ref"], {k: v.double().numpy() for k, v in s["forward"].items()}
    assert s["keys_on"] == set(s["off_before"][0].keys()) | set(GEO_KEYS)
    R = s["R"]
    assert got["depth_values"].shape == (R,) and got["depth_person_solo_level_list"].shape == (R, 2)
    out = s["on_geo"][0]
    assert all(out[DIFF[k]].requires_grad for k in GT.DIFF_KEYS)
    assert not out["depth_level_values"].requires_grad and not out["front_person"].requires_grad
    e_acc = np.abs(got["acc_person_solo_list"] - ref["acc_solo"]).max()
    e_dep = max(np.abs(got["depth_values"] - ref["depth"]).max(), np.abs(got["depth_person_list"] - ref["depth_person"]).max(),
                np.abs(got["depth_person_solo_list"] - ref["depth_solo"]).max())
    print(f"[geometry train] forward on the graph's tables: opacity |err| {e_acc:.3e}, depth sums |err| {e_dep:.3e}")
    assert e_acc <= TG.ACC and e_dep <= TG.DEPTH
    for tag, g, r, fe, mg, sl in (("merged", got["depth_level_values"], ref["depth_level"], ref["fe_cross"], ref["margin"], ref["slope"]),
                                  ("solo", got["depth_person_solo_level_list"].reshape(-1), ref["depth_solo_level"].reshape(-1),
                                   ref["fe_cross_solo"].reshape(-1), ref["margin_solo"].reshape(-1), ref["slope_solo"].reshape(-1))):
        ok = ~G.exempt(fe, mg)
        assert ((g == -1) == (r == -1))[ok].all(), tag
        c = ok & (r >= 0)
        err = np.abs(g - r)[c]
        print(f"[geometry train] forward {tag} level depth: max |err| {err.max() if len(err) else 0:.3e} over {int(c.sum())} crossings")
        assert (err <= TG.LEVEL[0] + TG.LEVEL[1] * sl[c]).all(), tag
    assert (got["front_person"][~G.exempt(ref["fe_cross"], ref["margin"])] == ref["front_person"][~G.exempt(ref["fe_cross"], ref["margin"])]).all()


def _rel_to_max(a, w):
    return (a.double() - w.double()).abs().max().item() / (w.abs().max().item() + 1e-12)


def test_flag_on_gradients_against_the_oracle():
    from tests import tolerances as T0
    s = _step()
    cross = s["oracle_forward"]["depth_solo_level"] >= 0
    print(f"[geometry train] {int(cross.sum())} of {cross.numel()} (ray, person) entries cross at level {s['model'].geometry_level} "
          f"in the oracle; {int(s['both'].sum())} rays where both do")
    assert cross.numel() == 242 and int(cross.sum()) >= 20
    for k in GT.DIFF_KEYS:
        e = float((s["forward"][DIFF[k]].double() - s["oracle_forward"][k]).abs().max())
        print(f"[geometry train] forward {DIFF[k]} against the oracle's sdf: max |err| {e:.3e}")
    _, got, body = s["on_geo"]
    first = "foreground_implicit_network_list.0.lin0.weight_v"
    first = first if first in got else sorted(k for k in got if "foreground_implicit_network_list.0" in k)[0]
    assert float(got[first].abs().max()) > 0, first
    worst = 0.0
    for k, w in s["oracle_params"].items():
        if k not in dict(s["model"].named_parameters()):
            continue
        a = got.get(k)
        if w is None:
            assert a is None or float(a.abs().max()) == 0.0, k
            continue
        assert a is not None, k
        a, b = a.cpu().double().reshape(-1), w.double().reshape(-1)
        rel = float((a - b).norm() / (b.norm() + 1e-12))
        worst = max(worst, rel)
        tol = T0.TRAIN_GRAD_REL_RENDERING if "rendering" in k else T0.TRAIN_GRAD_REL     # test_training_forward_loss_and_all_parameter_gradients
        assert rel < tol or float((a - b).abs().max()) < 1e-7, f"{k}: rel {rel:.3e} |g| {float(b.norm()):.3e}"
    print(f"[geometry train] geometry loss: worst relative parameter-gradient error {worst:.3e}")
    for k in BODY:
        e = _rel_to_max(body[k], s["oracle_body"][k])
        print(f"[geometry train] geometry loss: d / d {k}: rel-to-max err {e:.3e} (|want|max {s['oracle_body'][k].abs().max().item():.3e})")
        assert e < 5e-3, k


def test_geometry_and_colour_losses_add_up():
    """one backward with both losses = the sum of the two separate backwards: the geometry adjoint is accumulated after the
    compositing adjoint's store"""
    s = _step()
    _, pg, bg = s["on_geo"]
    _, pc, bc = s["on_colour"]
    _, pb, bb = s["on_both"]
    worst = 0.0
    for k in pb:
        want = pc[k] + pg[k]
        rel = float((pb[k] - want).norm() / (want.norm() + 1e-12))
        worst = max(worst, rel)
        assert rel < 1e-5 or float((pb[k] - want).abs().max()) < 1e-7, (k, rel)
    for k in BODY:
        want = bc[k] + bg[k]
        rel = float((bb[k] - want).norm() / (want.norm() + 1e-12))
        worst = max(worst, rel)
        assert rel < 1e-5, (k, rel)
    print(f"[geometry train] both losses vs the sum of the separate backwards: worst relative difference {worst:.3e}")
    # flag on, colour loss alone: the geometry outputs are unused, the step's gradients are the flag-off step's
    for k in pc:
        want = s["off_before"][1][k]
        assert float((pc[k] - want).norm() / (want.norm() + 1e-12)) < 1e-5 or float((pc[k] - want).abs().max()) < 1e-7, k


def test_ray_depth_order_step_against_the_oracle():
    s = _step()
    want, wb = s["oracle_order"]
    print(f"[geometry train] ray depth-order loss {s['order_loss']:.6f} (oracle {want:.6f}), active on {int(s['both'].sum())} rays")
    assert int(s["both"].sum()) > 0 and want > 0 and abs(s["order_loss"] - want) < 1e-4 * max(1.0, abs(want))
    for k in BODY:
        e = _rel_to_max(s["on_order"][2][k], wb[k])
        print(f"[geometry train] depth-order term: d / d {k}: rel-to-max err {e:.3e} (|want|max {wb[k].abs().max().item():.3e})")
        assert e < 5e-3, k


# ------------------------------------------------------------------------------------------------ 6. opt_depth_frame(depth_source='volume')
def test_depth_refinement_from_the_volume(monkeypatch):
    from multiply_amd import mesh as MESH
    from multiply_amd import mesh_losses as ML
    from multiply_amd import render as RENDER
    from multiply_amd.body_model_params import BodyModelParams
    s = _step()
    model, inp, R = s["model"], s["inp"], s["R"]

    def refuse(*a, **k):
        raise AssertionError("depth_source='volume' must not extract or rasterise a mesh")
    monkeypatch.setattr(MESH, "canonical_mesh", refuse)
    monkeypatch.setattr(RENDER.Renderer, "rasterize", refuse)
    bml = torch.nn.ModuleList()
    for p in range(2):
        bm = BodyModelParams(4, model_type="smpl").cuda()
        bm.init_parameters("betas", inp["smpl_shape"][0, p:p + 1].clone().cuda())
        bm.init_parameters("global_orient", inp["smpl_pose"][0, p, :3].repeat(4, 1).cuda())
        bm.init_parameters("body_pose", inp["smpl_pose"][0, p, 3:].repeat(4, 1).cuda())
        bm.init_parameters("transl", inp["smpl_trans"][0, p].repeat(4, 1).cuda())
        bml.append(bm)
    inputs = {k: inp[k].cuda() for k in ("intrinsics", "pose", "smpl_params", "idx")}
    inputs.update(P=torch.eye(4)[None].cuda(), C=torch.zeros(1, 3).cuda(), img_size=(11, 11))

    def sample_fn():
        return (dict(uv=inp["uv"].cuda(), index_outside=torch.zeros(R, dtype=torch.bool), sam_mask=s["labels"][None].cuda(),
                     hit_index=s["hit"]), dict(rgb=s["gt"]["rgb"]))
    t0 = [bm.transl.weight.detach().clone() for bm in bml]
    model.train_geometry = False
    with pytest.raises(ValueError):
        ML.opt_depth_frame(model, bml, s["loss_fn"], inputs, sample_fn, epoch=100, it_per_loop=1, lr=5e-3,
                           loss_opt={"interpenetration_loss_weight": 1}, depth_source="volume")
    hist = ML.opt_depth_frame(model, bml, s["loss_fn"], inputs, sample_fn, epoch=100, it_per_loop=3, lr=5e-3,
                              loss_opt={"depth_order_weight": 0.1}, depth_source="volume")
    torch.cuda.synchronize()
    assert model.train_geometry is False and model.training
    vals = [[float(h[k]) for k in ("render_loss", "depth_order_loss", "interpenetration_loss")] for h in hist]
    print("[geometry train] opt_depth_frame(volume): (render, depth-order, interpenetration) per iteration", vals)
    assert len(hist) == 3 and np.isfinite(vals).all() and all(v[1] != 0 for v in vals) and all(v[2] == 0 for v in vals)
    for p in range(2):
        moved = (bml[p].transl.weight.detach() - t0[p]).abs()
        assert float(moved[3].max()) > 1e-3 and float(moved[:3].max()) == 0.0           # the frame's row only
    model.train_geometry = True


# ------------------------------------------------------------------------------------------------ 7. person sharding
def test_person_sharded_training_refuses_the_flag():
    from multiply_amd import train as T
    s = _step()
    model = s["model"]
    assert model.train_geometry is True
    with pytest.raises(NotImplementedError, match="train_geometry"):
        T.forward_train(model, {**s["gin"], "hit_index": s["hit"]}, shard=(2, 0))
