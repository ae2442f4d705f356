"""The six layer-fused training launches (csrc/tfuse.hip: mp_tf_sdf_fwd / _bwd, mp_tf_bg_fwd / _bwd, mp_tf_col_fwd / _bwd) stage by
stage against their float64 restatement (tests/fused_train_reference.py), through the evaluator classes the trainer uses and in
the shipped arithmetic (TRAIN_PRECISION 'bf16x3'): outputs, every stash the weight-gradient contractions consume, every
parameter gradient, the adjoints of the inputs.

Every quantity q is held to  S(kernel q) <= max(4 S(model q), 2^-22)  (tests/tolerances_fused_train.py): S is the largest error
against the exact restatement relative to the element's column RMS (per-point tensors) or row maximum (parameter gradients), and
the model is the restatement under the kernels' documented roundings, evaluated on the same inputs in the same run.  The
reference takes the fp32 inputs -- points, conditioning, adjoints and the evaluator's own effective fp32 weights -- as exact.

Weights: person 0 of the `trained` regime (tests/weight_regimes.py); the geometric init is the control at 129 points.  Counts:
1, 16, 17, 127, 128, 129, 391 for every family (a workgroup owns 128 points, a wave 16).  Each case prints one `[parity]` line
per quantity: S(kernel), S(model), their ratio."""
import functools

import pytest
import torch

from tests import fused_train_reference as R
from tests import tolerances_fused_train as TOL

pytestmark = pytest.mark.gpu

CASES = [("trained", P) for P in R.COUNTS] + [("geometric", 129)]


@pytest.fixture(autouse=True)
def _shipped_arithmetic(monkeypatch):
    from multiply_amd import train as T
    monkeypatch.setattr(T, "TRAIN_PRECISION", "bf16x3")


@functools.lru_cache(maxsize=None)
def nets(regime):
    """the regime's networks, built once per module: (inputs and CPU modules, the same seeded modules on the device)"""
    return R.Nets(regime), R.build_networks(regime).cuda()


_REF = {}


def reference(key, fn):
    """(exact, model) of one case, computed once and shared (the weights of a regime are the same in every evaluator)"""
    if key not in _REF:
        _REF[key] = (fn(False), fn(True))
    return _REF[key]


def dev(t):
    return t.float().cuda().contiguous()


def f64(t):
    return t.detach().double().cpu()


class Parity:
    """collects S(kernel) against the bound for every quantity of a case; `check()` asserts them all at the end, so that a
    failing case still prints every line"""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def add(self, name, got, exact, model):
        k = R.kind_of(name)
        for label, rows in TOL.groups(name, k, exact[name]):
            g, e, m = (got, exact[name], model[name]) if rows is None else (got[rows], exact[name][rows], model[name][rows])
            s_k, s_m = TOL.S(g, e, k), TOL.S(m, e, k)
            b = TOL.bound(s_m)
            ratio = s_k / s_m if s_m > 0 else (0.0 if s_k == 0 else float("inf"))
            print(f"[parity] {self.tag} {label}: S(kernel) {s_k:.3e} S(model) {s_m:.3e} ratio {ratio:.2f} bound {b:.3e}")
            if not s_k <= b:
                self.bad.append((label, s_k, b))

    def check(self):
        assert not self.bad, f"{self.tag}: beyond max(4 S(model), 2^-22): {self.bad}"


def _stash(ev, t0, l):
    P = ev.P
    return f64(ev.arena[(t0 + l) * ev.R1:(t0 + l) * ev.R1 + 256 * P].view(P, 256))


def _block(ev, o, E):
    return f64(ev.arena[o:o + E * ev.P].view(ev.P, E))


def _weights(ev):
    return [f64(lw.W) for lw in ev.lins], [f64(lw.b) for lw in ev.lins]


def _param_grads(par, ev, dcond, exact, model):
    for l, lw in enumerate(ev.lins):
        par.add(f"dW_{l}", f64(lw.dW), exact, model)
        par.add(f"db_{l}", f64(lw.db), exact, model)
    par.add("dcond", f64(dcond), exact, model)


# ============================================================================================================== SDF net
def run_sdf(regime, P, tag):
    from multiply_amd import train as T
    N, m = nets(regime)
    net = m.foreground_implicit_network_list[0]
    x, cond, adj = N.sdf_case(P)
    ev = T.ImplicitTrainFused(net, dev(x), dev(cond))
    torch.cuda.synchronize()
    W, b = _weights(ev)
    exact, model = reference(("sdf", regime, P), lambda mdl: R.implicit_net("sdf", W, b, x, cond, adj, model=mdl, want_dx=True))
    par = Parity(f"sdf {regime} P {P}{tag}")
    # ---- forward: outputs and the stashes of both sweeps
    got = dict(sdf=f64(ev.sdf[:P]), feat=f64(ev.feat[:P]), grad=f64(ev.grad), IN=_block(ev, ev.o_IN, ev.E), G=_block(ev, ev.o_G, ev.E))
    for l in range(1, 9):
        got[f"X_{l}"] = _stash(ev, ev.t_X, l)             # (X_4 with its skip columns: _skip_features has run)
    for l in range(8):
        got[f"V_{l}"] = _stash(ev, ev.t_V, l)
    for name in R.SDF_POINT:
        par.add(name, got[name], exact, model)
    # ---- backward: adjoints on sdf, features and the gradient
    dcond = ev.backward(dev(adj["dfeat"]), dev(adj["dsdf"]), dev(adj["dgrad"]), want_dx=True)
    torch.cuda.synchronize()
    for l in range(8):
        par.add(f"dZ_{l}", _stash(ev, ev.t_dZ, l), exact, model)
    for l in range(1, 8):
        par.add(f"dT_{l}", _stash(ev, ev.t_dT, l), exact, model)
    _param_grads(par, ev, dcond, exact, model)
    par.add("dx", f64(ev.dx), exact, model)
    par.check()


@pytest.mark.parametrize("regime,P", CASES)
def test_sdf_forward_and_backward(regime, P):
    run_sdf(regime, P, "")


def test_sdf_backward_deterministic_form(monkeypatch):
    """the `_det` entry points (ordered sums instead of atomics) are held to the same bounds"""
    from multiply_amd import train as T
    monkeypatch.setattr(T, "_DET", [True])
    run_sdf("trained", 129, " det")


def test_sdf_points_adjoint():
    """d x of a term that reads the sdf column alone, the network held constant"""
    from multiply_amd import train as T
    P = 129
    N, m = nets("trained")
    x, cond, adj = N.sdf_case(P)
    ev = T.ImplicitTrainFused(m.foreground_implicit_network_list[0], dev(x), dev(cond))
    before = [(lw.dW.clone(), lw.db.clone()) for lw in ev.lins]
    dx = ev.points_adjoint(dev(adj["dsdf"]))
    torch.cuda.synchronize()
    W, b = _weights(ev)
    only = dict(dsdf=adj["dsdf"], dfeat=torch.zeros(P, 256, dtype=torch.float64), dgrad=torch.zeros(P, 3, dtype=torch.float64))
    exact, model = reference(("sdf points_adjoint", P), lambda mdl: R.implicit_net("sdf", W, b, x, cond, only, model=mdl, want_dx=True))
    par = Parity(f"sdf points_adjoint P {P}")
    par.add("dx", f64(dx), exact, model)
    par.check()
    for lw, (dW, db) in zip(ev.lins, before):
        assert torch.equal(lw.dW, dW) and torch.equal(lw.db, db), "no accumulator of the iteration is touched"


# ============================================================================================================== background net
def run_bg(regime, P, tag):
    from multiply_amd import train as T
    N, m = nets(regime)
    x, code, adj = N.bg_case(P)
    ev = T.ImplicitTrainFusedBG(m.bg_implicit_network, dev(x), dev(code))
    torch.cuda.synchronize()
    W, b = _weights(ev)
    exact, model = reference(("bg", regime, P), lambda mdl: R.implicit_net("bg", W, b, x, code, adj, model=mdl))
    par = Parity(f"bg {regime} P {P}{tag}")
    got = dict(sdf=f64(ev.sdf[:P]), feat=f64(ev.feat[:P]), IN=_block(ev, ev.o_IN, ev.E))
    for l in range(1, 9):
        got[f"X_{l}"] = _stash(ev, ev.t_X, l)
    for name in R.BG_POINT:
        par.add(name, got[name], exact, model)
    dcode = ev.backward(dev(adj["dfeat"]), dev(adj["dsdf"]))
    torch.cuda.synchronize()
    for l in range(8):
        par.add(f"dZ_{l}", _stash(ev, ev.t_dZ, l), exact, model)
    _param_grads(par, ev, dcode, exact, model)
    par.check()


@pytest.mark.parametrize("regime,P", CASES)
def test_background_forward_and_backward(regime, P):
    run_bg(regime, P, "")


def test_background_backward_deterministic_form(monkeypatch):
    from multiply_amd import train as T
    monkeypatch.setattr(T, "_DET", [True])
    run_bg("trained", 129, " det")


# ============================================================================================================== colour net
class _Dz4:
    """RenderTrainFused.backward keeps dz4 (the adjoint of the last layer's pre-activations) to itself: the test reads it where
    the evaluator hands it to the last layer's weight-gradient contraction (gemm_tn with M = 3)"""

    def __init__(self, T, monkeypatch):
        self.value, inner = None, T.gemm_tn

        def gemm_tn(A, lda, B, ldb, Cm, ldc, M, N, K, *rest):
            if M == 3 and torch.is_tensor(A):
                self.value = A
            return inner(A, lda, B, ldb, Cm, ldc, M, N, K, *rest)
        monkeypatch.setattr(T, "gemm_tn", gemm_tn)


def _colour(T, par, ren, XA, feat_t, n, cond, drgb, dfeat_t, ref_fn, dz4_tap, ref_key):
    """forward and backward of the fused colour evaluator on the features feat_t [>= n][256] (read in place), d feat written
    into dfeat_t; ref_fn(model, masks) -> the restatement.  Returns (rt, dXA, d pose8, exact, model)."""
    rt = T.RenderTrainFused(ren, XA, T._p(feat_t), 256, n, cond)
    torch.cuda.synchronize()
    NL = 256 * (n + 1)
    H = [f64(rt.stash[l * NL:l * NL + 256 * n].view(n, 256)) for l in range(4)]
    fwd_exact, fwd_model = reference(ref_key + ("fwd",), lambda mdl: ref_fn(mdl, None))
    par.add("rgb", f64(rt.rgb), fwd_exact, fwd_model)
    for l in range(4):
        par.add(f"H_{l}", H[l], fwd_exact, fwd_model)
    # the kernel's masks: equal to the float64 masks on every unit that is not ambiguous
    masks = [h > 0 for h in H]
    amb = R.ambiguous(fwd_exact, fwd_model)
    n_amb = sum(int(a.sum()) for a in amb)
    for l in range(4):
        differ = (masks[l] != (fwd_exact[f"Z_{l}"] > 0)) & ~amb[l]
        assert not bool(differ.any()), f"{par.tag}: layer {l}: ReLU mask differs from float64 on {int(differ.sum())} non-ambiguous units"
    print(f"[parity] {par.tag}: {n_amb} of {4 * 256 * n} units ambiguous, "
          f"{sum(int((masks[l] != (fwd_exact[f'Z_{l}'] > 0)).sum()) for l in range(4))} masks differ from float64")
    assert n_amb <= TOL.AMBIGUOUS_CAP * 4 * 256 * n
    exact, model = ref_fn(False, masks), ref_fn(True, masks)
    dXA = torch.full((n, 6), float("nan"), device="cuda")
    dh = rt.backward(drgb, dXA, T._p(dfeat_t), 256, feat_accumulate=False)
    torch.cuda.synchronize()
    par.add("dXA", f64(dXA), exact, model)
    par.add("dfeat", f64(dfeat_t[:n]), exact, model)
    par.add("dz4", f64(dz4_tap.value), exact, model)
    for l in range(4):
        par.add(f"dZ_{l}", f64(rt.stash[(4 + l) * NL:(4 + l) * NL + 256 * n].view(n, 256)), exact, model)
    for l, lw in enumerate(rt.lins):
        par.add(f"dW_{l}", f64(lw.dW), exact, model)
        par.add(f"db_{l}", f64(lw.db), exact, model)
    par.add("dpose8", f64(dh), exact, model)
    par.add("dlp_w", f64(rt.extra_grads[0]), exact, model)
    par.add("dlp_b", f64(rt.extra_grads[1]), exact, model)
    return rt, exact, model


def _colour_weights(T, ren, cond):
    """the evaluator's own effective fp32 weights (a throw-away refresh of the network's fused state)"""
    cs = T.fused_state("col", ren, None).refresh(cond)
    torch.cuda.synchronize()
    return [f64(lw.W) for lw in cs.lins], [f64(lw.b) for lw in cs.lins], f64(cs.lp_w), f64(cs.lp_b)


def run_colour(regime, n, tag, monkeypatch):
    from multiply_amd import train as T
    N, m = nets(regime)
    ren = m.foreground_rendering_network_list[0]
    XA, feat, cond, drgb = N.colour_case(n)
    W, b, lp_w, lp_b = _colour_weights(T, ren, dev(cond))
    ref_fn = lambda mdl, masks: R.colour_net(W, b, lp_w, lp_b, XA, feat[:n], cond, drgb if masks is not None else None, masks, model=mdl)
    feat_t = dev(feat)                                     # n + 7 rows: more rows than points, like the SDF net's batch
    feat_0 = feat_t.clone()
    dfeat_t = torch.full((n + 7, 256), 7.0, device="cuda")
    par = Parity(f"col {regime} n {n}{tag}")
    _colour(T, par, ren, dev(XA), feat_t, n, dev(cond), dev(drgb), dfeat_t, ref_fn, _Dz4(T, monkeypatch), ("col", regime, n))
    assert bool((dfeat_t[n:] == 7.0).all()) and torch.equal(feat_t, feat_0), "rows past the n points come back untouched"
    par.check()


@pytest.mark.parametrize("regime,n", CASES)
def test_colour_forward_and_backward(regime, n, monkeypatch):
    run_colour(regime, n, "", monkeypatch)


# ============================================================================================================== the chain
def test_chain_sdf_colour_colour_backward_sdf_backward(monkeypatch):
    """the trainer's chain at P = 200, n = 150: the colour net reads the SDF evaluator's first n feature rows in place, its
    backward writes them into new_dfeat(n), the SDF backward consumes that.  Every gradient of both nets against the float64
    chain (model: the chain under the kernels' roundings)."""
    from multiply_amd import train as T
    P, n = 200, 150
    N, m = nets("trained")
    net, ren = m.foreground_implicit_network_list[0], m.foreground_rendering_network_list[0]
    x, cond, adj = N.sdf_case(P)
    XA, _, _, drgb = N.colour_case(n)
    ev = T.ImplicitTrainFused(net, dev(x), dev(cond))
    torch.cuda.synchronize()
    W, b = _weights(ev)
    Wc, bc, lp_w, lp_b = _colour_weights(T, ren, dev(cond))
    fwd = {mdl: R.implicit_net("sdf", W, b, x, cond, model=mdl) for mdl in (False, True)}
    ref_fn = lambda mdl, masks: R.colour_net(Wc, bc, lp_w, lp_b, XA, fwd[mdl]["feat"][:n], cond, drgb if masks is not None else None,
                                             masks, model=mdl)
    par = Parity(f"chain colour P {P} n {n}")
    feat_0 = ev.feat.clone()
    dfeat_t = ev.new_dfeat(n)
    ptr, ld, accumulate = ev.dfeat_target(dfeat_t)
    assert ld == 256 and not accumulate
    _, c_exact, c_model = _colour(T, par, ren, dev(XA), ev.feat, n, dev(cond), dev(drgb), dfeat_t, ref_fn, _Dz4(T, monkeypatch),
                                  ("chain", P, n))
    assert torch.equal(ev.feat, feat_0) and not bool(dfeat_t[n:].any())
    par.check()
    par = Parity(f"chain sdf P {P} n {n}")
    ref = {}
    for mdl, col in ((False, c_exact), (True, c_model)):
        a = dict(adj, dfeat=torch.cat([col["dfeat"], torch.zeros(P - n, 256, dtype=torch.float64)]))
        ref[mdl] = R.implicit_net("sdf", W, b, x, cond, a, model=mdl, want_dx=True)
    dcond = ev.backward(dfeat_t, dev(adj["dsdf"]), dev(adj["dgrad"]), want_dx=True)
    torch.cuda.synchronize()
    _param_grads(par, ev, dcond, ref[False], ref[True])
    par.add("dx", f64(ev.dx), ref[False], ref[True])
    par.check()


# ============================================================================================================== stale arena
@pytest.mark.parametrize("P", [129, 17])
def test_no_result_depends_on_stale_arena_contents(P, monkeypatch):
    """The arenas come from torch.empty (train._big_empty): every iteration sees whatever the last one left there.  Here they
    arrive full of NaN -- the SDF and background arenas and the colour stash -- and every quantity asserted above is still finite
    and inside its bound.  (The pad row P of a stash tensor may hold anything: it is never read back into a result.)"""
    from multiply_amd import train as T
    inner = T._big_empty

    def nan_empty(*a, **k):
        return inner(*a, **k).fill_(float("nan"))
    monkeypatch.setattr(T, "_big_empty", nan_empty)
    run_sdf("trained", P, " stale")
    run_bg("trained", P, " stale")
    run_colour("trained", P, " stale", monkeypatch)
