"""The float64 reference of the fused training kernels and its inputs, checked without a GPU:
  * the exact restatement (tests/fused_train_reference.py, model=False) against float64 autograd on the oracle's formulas;
  * the error statistic S has POWER: nine value-only mutations of the restatement each show at >= 10 x the bound the GPU test
    holds the kernels to, at every point count where the mutation applies;
  * the colour net's ReLU masks are well defined: at most 0.1 % of its hidden units are ambiguous."""
import functools

import pytest
import torch

from oracle import multiply_oracle as O
from tests import fused_train_reference as R
from tests import tolerances_fused_train as TOL


@functools.lru_cache(maxsize=None)
def nets(regime):
    return R.Nets(regime)


@functools.lru_cache(maxsize=None)
def runs(regime, family, P):
    """(exact, model) of one family at P points: shared by the tests below, never modified"""
    return _run(regime, family, P, model=False), _run(regime, family, P, model=True)


def _run(regime, family, P, model=False, mutate=None):
    N = nets(regime)
    if family == "col":
        W, b = N.weights("col")
        XA, feat, cond, drgb = N.colour_case(P)
        return R.colour_net(W, b, *N.lin_pose(), XA, feat[:P], cond, drgb, model=model, mutate=mutate)
    W, b = N.weights(family)
    x, cond, adj = N.sdf_case(P) if family == "sdf" else N.bg_case(P)
    return R.implicit_net(family, W, b, x, cond, adj, model=model, want_dx=True, mutate=mutate)


def _rel(name, got, want):
    e = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-300)
    assert e <= 1e-11, (name, e)
    return e


def _eff_sd(W, b, grad=True):
    sd = {}
    for l, (w, bb) in enumerate(zip(W, b)):
        sd[f"n.lin{l}.weight"] = w.clone().requires_grad_(grad)
        sd[f"n.lin{l}.bias"] = bb.clone().requires_grad_(grad)
    return sd


@pytest.mark.parametrize("P", [1, 17, 129])
@pytest.mark.parametrize("regime", ["trained", "geometric"])
def test_restatement_against_autograd(regime, P):
    """every output and every parameter / input gradient of the three restatements, relative 1e-11 of the tensor's maximum"""
    N = nets(regime)
    worst = 0.0
    for family in ("sdf", "bg"):
        W, b = N.weights(family)
        x, cond, adj = N.sdf_case(P) if family == "sdf" else N.bg_case(P)
        got = runs(regime, family, P)[0]
        sd = _eff_sd(W, b)
        xg, cg = x.clone().requires_grad_(True), cond.clone().requires_grad_(True)
        out = O.implicit_forward(sd, "n.", xg, cg, R.CFG[family]["L"])
        loss = (out[:, 0] * adj["dsdf"]).sum() + (out[:, 1:] * adj["dfeat"]).sum()
        worst = max(worst, _rel("sdf", got["sdf"], out[:, 0].detach()), _rel("feat", got["feat"], out[:, 1:].detach()))
        if family == "sdf":
            g = torch.autograd.grad(out[:, 0].sum(), xg, create_graph=True)[0]
            loss = loss + (g * adj["dgrad"]).sum()
            worst = max(worst, _rel("grad", got["grad"], g.detach()))
        wrt = [sd[f"n.lin{l}.weight"] for l in range(9)] + [sd[f"n.lin{l}.bias"] for l in range(9)] + [cg] + ([xg] if family == "sdf" else [])
        want = torch.autograd.grad(loss, wrt)
        for name, w in zip(R.NET_PARAM + ["dx"], want):
            worst = max(worst, _rel(f"{family} {name}", got[name], w))
    W, b = N.weights("col")
    lp_w, lp_b = N.lin_pose()
    XA, feat, cond, drgb = N.colour_case(P)
    got = runs(regime, "col", P)[0]
    sd = _eff_sd(W, b)
    sd["n.lin_pose.weight"], sd["n.lin_pose.bias"] = lp_w.clone().requires_grad_(True), lp_b.clone().requires_grad_(True)
    XAg, fg, cg = XA.clone().requires_grad_(True), feat[:P].clone().requires_grad_(True), cond.clone().requires_grad_(True)
    rgb = O.rendering_forward_pose_no_view(sd, "n.", XAg[:, :3], XAg[:, 3:], cg, fg)
    worst = max(worst, _rel("rgb", got["rgb"], rgb.detach()))
    names = [f"dW_{l}" for l in range(5)] + [f"db_{l}" for l in range(5)] + ["dlp_w", "dlp_b", "dXA", "dfeat", "dcond"]
    wrt = [sd[f"n.lin{l}.weight"] for l in range(5)] + [sd[f"n.lin{l}.bias"] for l in range(5)] + \
        [sd["n.lin_pose.weight"], sd["n.lin_pose.bias"], XAg, fg, cg]
    for name, w in zip(names, torch.autograd.grad((rgb * drgb).sum(), wrt)):
        worst = max(worst, _rel(f"col {name}", got[name], w))
    # d pose8 and dz4 are no autograd leaves: through the identities d lin_pose.bias = d pose8, dz4 = d rgb . rgb (1 - rgb)
    y = rgb.detach()
    worst = max(worst, _rel("col dz4", got["dz4"], drgb * y * (1 - y)))
    print(f"[restatement] {regime} P {P}: worst relative distance to float64 autograd {worst:.2e}")


@pytest.mark.parametrize("key", sorted(R.MUTATIONS))
@pytest.mark.parametrize("P", R.COUNTS)
def test_mutation_is_seen_at_ten_times_the_bound(P, key):
    """S(mutant) >= 10 x max(4 S(model), 2^-22) on the quantity named in R.MUTATIONS -- for a parameter-gradient matrix on one
    of its two groups of rows (TOL.groups) -- `trained` weights, every count.

    Grouping: (a) is read on db_5 (on dZ_5 itself the factor is about 1 at one point, where a column's RMS is the element);
    (i) on the large rows of the background dW_4: pooled with the small rows the factor is 0.2 at one point, because S(model)
    is then the relative error of the elements of dZ_4 = sigma'_4 (.) dX_5 whose sum dX_5 cancels (1.3e-2 against the
    mutation's 1.0e-2)."""
    family, what, name = R.MUTATIONS[key]
    if key == "f" and P < 2:
        return                                         # (one point has no previous point: the mutation does not apply)
    exact, model = runs("trained", family, P)
    mut = _run("trained", family, P, mutate=key)
    k = R.kind_of(name)
    best = 0.0
    for label, rows in TOL.groups(name, k, exact[name]):
        u, e, m = (mut[name], exact[name], model[name]) if rows is None else (mut[name][rows], exact[name][rows], model[name][rows])
        s_mut, s_model = TOL.S(u, e, k), TOL.S(m, e, k)
        b = TOL.bound(s_model)
        best = max(best, s_mut / b)
        print(f"[power] P {P} ({key}) {what}: {label} S(mutant) {s_mut:.3e}, S(model) {s_model:.3e}, bound {b:.3e}, factor {s_mut / b:.1f}")
    assert best >= TOL.POWER, (key, what, name, best)


@pytest.mark.parametrize("regime,n", [("trained", n) for n in R.COUNTS] + [("geometric", 129)])
def test_relu_ambiguity_cap(regime, n):
    exact, model = runs(regime, "col", n)
    amb = R.ambiguous(exact, model)
    share = sum(int(a.sum()) for a in amb) / (4 * 256 * n)
    rms = [float(exact[f"Z_{l}"].pow(2).mean().sqrt()) for l in range(4)]
    print(f"[ambiguity] {regime} n {n}: {sum(int(a.sum()) for a in amb)} of {4 * 256 * n} units ambiguous ({share:.2e}); pre-activation RMS {rms}")
    assert share <= TOL.AMBIGUOUS_CAP
