"""The element-wise / small kernels of the training path (csrc/train.hip, mp_tr_*) called directly, each against the float64
reference and the per-element bound of tests/train_elementwise_reference.py (limits: tests/tolerances_train_elementwise.py),
or bit for bit where the result is exact.  Operands sit in NaN-surrounded buffers and outputs in sentinel-surrounded windows
that start out NaN (tests/gemm_reference.py: Embedded, GuardedC, GuardedVec): a read past an operand, an element left
unwritten and a write outside the window all show.  The shapes are the smallest at which the kernels can go wrong: column
counts around the float4 width, rows around the 256-thread block and the 64-lane wave, odd strides, unaligned bases."""
import ctypes as C
import itertools
import math

import pytest
import torch

from tests import gemm_reference as G
from tests import tolerances_train_elementwise as TOL
from tests import train_elementwise_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
RS2 = R.f32(1 / math.sqrt(2))
WORST = {}


def _hip():
    from multiply_amd import hip
    return hip


def _vp(p):
    return None if p is None else C.c_void_p(int(p))


def _in(x, ld=None, off=0):
    """a float operand [rows][...] (1-D: one row) in a NaN-surrounded buffer"""
    x2 = x.reshape(1, -1) if x.dim() == 1 else x.reshape(x.shape[0], -1)
    return G.Embedded(x2.to(DEV), x2.shape[1] if ld is None else ld, off)


def _out(rows, cols, ld=None, col0=0, init=None):
    """an output window [rows][cols]; init None: NaN (an element left unwritten fails every comparison)"""
    c0 = torch.full((rows, cols), float("nan")) if init is None else init.reshape(rows, cols)
    return G.GuardedC(c0.to(DEV), cols + col0 if ld is None else ld, col0)


def _vec(n, off=0, init=None):
    return G.GuardedVec((torch.full((n,), float("nan")) if init is None else init).to(DEV), off)


def _i32(t):
    return t.to(torch.int32).to(DEV).contiguous()


def _check(kernel, inp, got):
    """every output of `got` (device tensors) within limit(kernel) x bound of the float64 reference"""
    rb = inp.setdefault("_rb", {})                              # reference and bound: once per case, shared by its layouts
    if kernel not in rb:
        rb[kernel] = (R.reference(kernel, inp), R.bounds(kernel, inp))
    ref, bnd = rb[kernel]
    rs = {k: R.worst_ratio(v.cpu(), ref[k], bnd[k].expand_as(ref[k])) for k, v in got.items()}
    assert set(rs) == set(bnd), (set(rs), set(bnd))
    for k, r in rs.items():
        WORST[kernel] = max(WORST.get(kernel, 0.0), r)
        assert r <= TOL.limit(kernel), (kernel, k, r, TOL.limit(kernel))
    return rs


def _report(*kernels):
    for k in kernels:
        print(f"RATIO {k} {WORST.get(k, float('nan')):.4g} (limit {TOL.limit(k):.3g})")


# ============================================================================================== the five dispatched entry points
ENTRY = {"softplus_fwd": (("Z",), ("H",)), "relu_bwd": (("H", "dH"), ("dZ",)), "sigmul": (("Z", "U"), ("V",)),
         "rev_adj": (("Z", "U", "dV"), ("dU", "dS")), "dz": (("Z", "dX", "dS"), ("dZ",))}
ROWS5 = (1, 3, 64, 257)
C5 = (1, 3, 4, 8, 252, 256)


def _inputs5(entry, rows, Cc, seed, use_U=True):
    if entry == "softplus_fwd":
        return R.case_softplus(rows, Cc, 0, seed, RS2)
    if entry == "relu_bwd":
        H = R.softplus_z(rows, Cc, seed)                       # zeros, both signs, tiny values
        return {"H": H, "dH": R.randn((rows, Cc), seed + 1)}
    return R.case_rev(rows, Cc, seed, use_U)


def _launch5(entry, inp, ld, off, col0=0):
    """places the operands (ld / off: {argument: row stride / float offset of the base}; default C and 0), calls the entry
    point -> ({output: window clone}, the predicate's clauses {name: bool})"""
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    ins, outs = ENTRY[entry]
    rows, Cc = inp[ins[0]].shape
    E, ptr, lds = {}, {}, {}
    for a in ins:
        if a == "U" and inp["U"] is None:
            E["wrow"] = _in(inp["wrow"], None, off.get("wrow", 0))
            ptr["wrow"] = E["wrow"].data_ptr()
            continue
        E[a] = _in(inp[a], ld.get(a, Cc), off.get(a, 0))
        ptr[a], lds[a] = E[a].data_ptr(), E[a].ld
    O = {}
    for a in outs:
        c = col0 if entry == "softplus_fwd" else 0
        ldc, o = ld.get(a, Cc + c), off.get(a, 0)
        if (-ldc) % 4 + o + c + Cc <= ldc:                      # the window starts one guard row in: undo what ldc does to the
            o += (-ldc) % 4                                     # base's alignment, so that `off` alone decides it
        O[a] = _out(rows, Cc, ldc, o + c)
        ptr[a], lds[a] = O[a].data_ptr() - 4 * c, ldc
    cl = {"C": Cc % 4 == 0}
    cl.update({"al:" + a: p % 16 == 0 for a, p in ptr.items()})
    cl.update({"ld:" + a: l % 4 == 0 for a, l in lds.items()})
    if entry == "softplus_fwd":
        cl["col0"] = col0 % 4 == 0
    p = {a: _vp(v) for a, v in ptr.items()}
    if entry == "softplus_fwd":
        L.mp_tr_softplus_fwd(p["Z"], lds["Z"], rows, Cc, 0, inp["scale"], p["H"], lds["H"], col0, st)
    elif entry == "relu_bwd":
        L.mp_tr_relu_bwd(p["H"], lds["H"], rows, Cc, p["dH"], lds["dH"], p["dZ"], lds["dZ"], st)
    elif entry == "sigmul":
        L.mp_tr_sigmul(p["Z"], lds["Z"], rows, Cc, p.get("U"), lds.get("U", 0), p.get("wrow"), inp["scale"], p["V"], lds["V"], st)
    elif entry == "rev_adj":
        L.mp_tr_rev_adj(p["Z"], lds["Z"], rows, Cc, p.get("U"), lds.get("U", 0), p.get("wrow"), inp["uscale"], p["dV"],
                        lds["dV"], p["dU"], lds["dU"], p["dS"], lds["dS"], st)
    else:
        L.mp_tr_dz(p["Z"], lds["Z"], rows, Cc, p["dX"], lds["dX"], inp["scale"], p["dS"], lds["dS"], p["dZ"], lds["dZ"], st)
    return {a: O[a].check() for a in outs}, cl


def _verify5(entry, inp, got):
    if entry == "relu_bwd":
        want = torch.where(inp["H"] > 0, inp["dH"], torch.zeros_like(inp["dH"]))
        assert torch.equal(got["dZ"].cpu(), want)
    else:
        _check(entry, inp, got)


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


@pytest.mark.parametrize("entry", list(ENTRY))
def test_dispatched_shapes_and_strides(entry):
    """rows x C x {contiguous, ld = C + 4, ld odd}; contiguous with C % 4 == 0 must satisfy the float4 predicate, an odd ld must
    not, and wherever both kernels serve the same values their results agree bit for bit"""
    n_run = n_f4 = n_scalar = 0
    ins, outs = ENTRY[entry]
    for si, (rows, Cc) in enumerate(itertools.product(ROWS5, C5)):
        inp = _inputs5(entry, rows, Cc, 1000 + 10 * si)
        res = {}
        for name, ldf in (("contiguous", lambda c: c), ("ld+4", lambda c: c + 4), ("ld odd", _odd)):
            got, cl = _launch5(entry, inp, {a: ldf(Cc) for a in ins + outs}, {})
            f4 = all(cl.values())
            if name == "contiguous":
                assert f4 == (Cc % 4 == 0), cl
            if name == "ld odd":
                assert not f4 and not cl["ld:" + outs[0]], cl
            _verify5(entry, inp, got)
            res[name] = (got, f4)
            n_run += 1
            n_f4 += f4
            n_scalar += not f4
        if res["contiguous"][1]:
            assert not res["ld odd"][1]
            assert _same_bits(res["contiguous"][0], res["ld odd"][0]) and _same_bits(res["contiguous"][0], res["ld+4"][0]), (rows, Cc)
    assert n_run == 72 and n_f4 >= 32 and n_scalar >= 32
    if entry != "relu_bwd":
        _report(entry)


def _odd(k):
    return k + 1 if k % 2 == 0 else k + 2


@pytest.mark.parametrize("entry", list(ENTRY))
def test_dispatch_predicate_clause_by_clause(entry):
    """every clause of the float4 predicate as the SOLE reason for the one-element kernel: one argument's ld odd, one
    argument's base one float off, C = 3 inside aligned rows of 4, col0 = 2 (col0 = 4 stays float4), wrow one float off with U
    NULL; each result equals the float4 kernel's bit for bit.  (fits32, the predicate's last clause, needs 2^33 elements to fail.)"""
    ins, outs = ENTRY[entry]
    covered, n_run = set(), 0
    variants = [True, False] if "U" in ins else [True]
    for (rows, Cc), use_U in itertools.product(((3, 8), (64, 256)), variants):
        inp = _inputs5(entry, rows, Cc, 2000 + rows + (0 if use_U else 1), use_U)
        args = [a for a in ins + outs if not (a == "U" and not use_U)]
        base = {a: Cc + 4 for a in args}
        if entry == "softplus_fwd":
            base["H"] = Cc + 8
        ref_got, cl = _launch5(entry, inp, base, {})
        assert all(cl.values()), cl
        _verify5(entry, inp, ref_got)
        cases = [("ld:" + a, dict(base, **{a: base[a] + 1}), {}, 0) for a in args]
        cases += [("al:" + a, base, {a: 1}, 0) for a in args]
        if not use_U:
            cases.append(("al:wrow", base, {"wrow": 1}, 0))
        if entry == "softplus_fwd":
            cases.append(("col0", base, {}, 2))
        for clause, ld, off, col0 in cases:
            got, cl = _launch5(entry, inp, ld, off, col0)
            assert [k for k, v in cl.items() if not v] == [clause], (clause, cl)
            _verify5(entry, inp, got)
            assert _same_bits(ref_got, got), (entry, clause)
            covered.add(clause)
            n_run += 1
        if entry == "softplus_fwd":
            got, cl = _launch5(entry, inp, base, {}, 4)
            assert all(cl.values()) and _same_bits(ref_got, got)
    # C % 4: three columns inside aligned rows of four
    inp = _inputs5(entry, 5, 3, 2100)
    got, cl = _launch5(entry, inp, {a: 4 for a in ins + outs}, {})
    assert [k for k, v in cl.items() if not v] == ["C"], cl
    _verify5(entry, inp, got)
    covered.add("C")
    want = {"C"} | {"ld:" + a for a in ins + outs} | {"al:" + a for a in ins + outs}
    if "U" in ins:
        want.add("al:wrow")
    if entry == "softplus_fwd":
        want.add("col0")
    assert covered == want, (covered ^ want)
    assert n_run >= 2 * (len(want) - 2)


def test_rev_adj_then_dz_is_the_adjoint_of_both_sweeps():
    """dz(Z, dX, scale, dS of rev_adj) against autograd of sum s(Z) scale dX + sum s'(Z) U uscale dV w.r.t. Z"""
    n_run = 0
    for (rows, Cc), use_U in itertools.product(((3, 3), (64, 8), (257, 4)), (True, False)):
        inp = R.case_rev(rows, Cc, 2200 + rows, use_U)
        inp["scale"] = inp["uscale"]
        got, _ = _launch5("rev_adj", inp, {}, {})
        chained = {k: v for k, v in dict(inp, dS=got["dS"].cpu()).items() if k != "_rb"}
        got2, _ = _launch5("dz", chained, {}, {})
        _check("rev_chain", inp, got2)
        n_run += 1
    assert n_run == 6
    _report("rev_chain")


# ======================================================================================================== forward-mode softplus
def test_softplus_forward_mode_and_adjoint():
    """P > 0 (rows = 4P: value rows, then the tangent blocks k P + r) and P = 0, windows at col0 with ld > C"""
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for P, Cc, (pad, col0) in itertools.product((0, 1, 5, 64), (3, 8), ((0, 0), (5, 5))):
        rows = 4 * P if P else 7
        inp = R.case_softplus(rows, Cc, P, 3000 + 10 * P + Cc, RS2)
        Z = _in(inp["Z"], Cc + pad)
        H = _out(rows, Cc, Cc + col0 + pad, col0)
        L.mp_tr_softplus_fwd(_vp(Z.data_ptr()), Z.ld, rows, Cc, P, inp["scale"], _vp(H.data_ptr() - 4 * col0), H.ldc, col0, st)
        _check("softplus_fwd", inp, {"H": H.check()})
        dH = _in(inp["dH"], Cc + col0 + pad, col0)                # the adjoints sit in the same window layout
        dZ = _out(rows, Cc, Cc + pad + 1)
        L.mp_tr_softplus_bwd(_vp(Z.data_ptr()), Z.ld, rows, Cc, P, inp["scale"], _vp(dH.data_ptr() - 4 * col0), dH.ld, col0,
                             _vp(dZ.data_ptr()), dZ.ldc, st)
        _check("softplus_bwd", inp, {"dZ": dZ.check()})
        n_run += 1
    assert n_run == 16
    _report("softplus_fwd", "softplus_bwd")


# ============================================================================================================= Fourier features
PE_L = (0, 1, 4, 6, 10)
PE_P = (1, 255, 256, 257)


def test_pe_and_its_adjoint():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for (D, fwd, col0, scale), Lo, P in itertools.product(((3, 1, 5, RS2), (4, 0, 0, 1.0), (3, 0, 5, 1.0), (4, 0, 5, RS2), (3, 1, 0, 1.0)),
                                                          PE_L, PE_P):
        inp = R.case_pe(P, D, Lo, fwd, scale, 4000 + 7 * Lo + P)
        NF, rows = R.pe_width(D, Lo), (4 * P if fwd else P)
        x = _in(inp["x"])
        out = _out(rows, NF, col0 + NF + 3, col0)
        L.mp_tr_pe(_vp(x.data_ptr()), D, P, Lo, fwd, inp["scale"], _vp(out.data_ptr() - 4 * col0), out.ldc, col0, st)
        _check("pe", inp, {"out": out.check()})
        dIN = _in(inp["dIN"], NF + 2)
        dx = _out(P, D, init=inp["dx0"])
        L.mp_tr_pe_bwd(_vp(x.data_ptr()), D, P, Lo, fwd, _vp(dIN.data_ptr()), dIN.ld, _vp(dx.data_ptr()), st)
        _check("pe_bwd", inp, {"dx": dx.check()})
        n_run += 1
    assert n_run == 100
    _report("pe", "pe_bwd")


def test_pe_grad_and_its_adjoint():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for Lo, P, with_dx in itertools.product(PE_L, PE_P, (True, False)):
        inp = R.case_pe_grad(P, Lo, 4500 + 7 * Lo + P, with_dx)
        NF = R.pe_width(3, Lo)
        x, Gm, dgrad = _in(inp["x"]), _in(inp["G"], NF + 1), _in(inp["dgrad"])
        grad = _out(P, 3)
        L.mp_tr_pe_grad_fwd(_vp(x.data_ptr()), P, Lo, _vp(Gm.data_ptr()), Gm.ld, _vp(grad.data_ptr()), st)
        _check("pe_grad_fwd", inp, {"grad": grad.check()})
        dG = _out(P, NF, NF + 4)
        dx = _out(P, 3, init=inp["dx0"]) if with_dx else None
        L.mp_tr_pe_grad_bwd(_vp(x.data_ptr()), P, Lo, _vp(dgrad.data_ptr()), _vp(Gm.data_ptr()), Gm.ld, _vp(dG.data_ptr()), dG.ldc,
                            _vp(dx.data_ptr()) if with_dx else None, st)
        got = {"dG": dG.check()}
        if with_dx:
            got["dx"] = dx.check()
        _check("pe_grad_bwd", inp, got)
        n_run += 1
    assert n_run == 40
    _report("pe_grad_fwd", "pe_grad_bwd")


# ================================================================================================================== weight norm
WN_SHAPES = ((1, 1), (3, 39), (8, 63), (8, 64), (8, 65), (256, 257), (5, 270))


def _wn_single(inp, with_wt=True):
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    o, i = inp["v"].shape
    v, dW = _in(inp["v"]), _in(inp["dW"])
    g = None if inp["g"] is None else _in(inp["g"])
    W, WT = _out(o, i), (_out(i, o) if with_wt else None)
    L.mp_tr_wn_fwd(_vp(v.data_ptr()), _vp(g.data_ptr()) if g else None, o, i, _vp(W.data_ptr()),
                   _vp(WT.data_ptr()) if with_wt else None, st)
    dv = _out(o, i)
    dg = _vec(o, 3) if g else None
    L.mp_tr_wn_bwd(_vp(v.data_ptr()), _vp(g.data_ptr()) if g else None, o, i, _vp(dW.data_ptr()), _vp(dv.data_ptr()),
                   _vp(dg.data_ptr()) if g else None, st)
    got = {"W": W.check(), "dv": dv.check()}
    if with_wt:
        got["WT"] = WT.check()
    if g:
        got["dg"] = dg.check()
    return got


def test_weight_norm_single_layer():
    n_run = 0
    for si, ((o, i), with_g, with_wt) in enumerate(itertools.product(WN_SHAPES, (True, False), (True, False))):
        inp = R.case_wn(o, i, 5000 + si, with_g)
        if not with_g:
            inp["dW"] = R.ints((o, i), 5000 + si)
        got = _wn_single(inp, with_wt)
        if with_wt:
            assert torch.equal(got["WT"], got["W"].T)
        if with_g:
            _check("wn_fwd", inp, {"W": got["W"]})
            _check("wn_bwd", inp, {"dv": got["dv"], "dg": got["dg"]})
        else:                                                    # no weight norm: both directions are pure copies
            assert torch.equal(got["W"].cpu(), inp["v"]) and torch.equal(got["dv"].cpu(), inp["dW"])
        n_run += 1
    assert n_run == 28
    _report("wn_fwd", "wn_bwd")


def _wn_multi_shapes(n):
    if n == 1:
        return [(8, 65)]
    if n == 2:
        return [(1, 1), (3, 39)]
    if n == 7:
        return [(1, 1), (1, 1), (3, 39), (8, 63), (8, 64), (5, 270), (1, 1)]
    cyc = [(3, 39), (8, 63), (1, 1), (1, 1), (8, 64), (8, 65), (5, 270)]
    return [(1, 1)] + [cyc[k % len(cyc)] for k in range(37)] + [(256, 257), (1, 1)]


@pytest.mark.parametrize("n_desc", (1, 2, 7, 40))
def test_weight_norm_many_layers_equal_single_layers_bit_for_bit(n_desc):
    from multiply_amd.train import MpWnDesc
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    shapes = _wn_multi_shapes(n_desc)
    assert len(shapes) == n_desc
    with_g = [li % 3 != 1 for li in range(n_desc)]
    row0, total, dW_off, dv_off, dg_off, acc_n, grad_n = R.wn_layout(shapes, with_g, 17 + n_desc)
    cases = [R.case_wn(o, i, 5200 + 3 * li, with_g[li]) for li, (o, i) in enumerate(shapes)]
    singles = [_wn_single(c) for c in cases]
    acc = torch.full((acc_n + 8,), float("nan"), device=DEV)
    gbits = torch.full((grad_n + 8,), G.SENTINEL, dtype=torch.int32, device=DEV)
    grad = gbits.view(torch.float32)
    written = torch.zeros(grad_n + 8, dtype=torch.bool, device=DEV)
    keep, arr = [], (MpWnDesc * n_desc)()
    for li, ((o, i), c) in enumerate(zip(shapes, cases)):
        v, g = _in(c["v"]), (_in(c["g"]) if with_g[li] else None)
        W, WT = _out(o, i), (_out(i, o) if li % 2 == 0 else None)
        keep.append((v, g, W, WT))
        acc[dW_off[li]:dW_off[li] + o * i] = c["dW"].reshape(-1).to(DEV)
        written[dv_off[li]:dv_off[li] + o * i] = True
        if with_g[li]:
            written[dg_off[li]:dg_off[li] + o] = True
        arr[li] = MpWnDesc(v.data_ptr(), g.data_ptr() if g else None, W.data_ptr(), WT.data_ptr() if WT else None, dW_off[li],
                           dv_off[li], dg_off[li] if with_g[li] else 0, o, i, row0[li], 0)
    descs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.mp_tr_wn_fwd_multi(_vp(descs.data_ptr()), n_desc, total, st)
    L.mp_tr_wn_bwd_multi(_vp(descs.data_ptr()), n_desc, total, _vp(acc.data_ptr()), _vp(grad.data_ptr()), st)
    torch.cuda.synchronize()
    assert bool((gbits[~written] == G.SENTINEL).all()), "a write landed between the gradient blocks"
    want_W = R.ref_wn_fwd_multi([(c["v"], c["g"]) for c in cases], row0, total)
    for li, ((o, i), c, s) in enumerate(zip(shapes, cases, singles)):
        v, g, W, WT = keep[li]
        Wm = W.check()
        assert torch.equal(Wm.view(torch.int32), s["W"].view(torch.int32)), ("W", li)
        if WT is not None:
            assert torch.equal(WT.check(), Wm.T), ("WT", li)
        dv = grad[dv_off[li]:dv_off[li] + o * i].view(o, i)
        assert torch.equal(dv.view(torch.int32), s["dv"].view(torch.int32)), ("dv", li)
        if with_g[li]:
            assert torch.equal(grad[dg_off[li]:dg_off[li] + o].view(torch.int32), s["dg"].view(torch.int32)), ("dg", li)
            bound = R.bounds("wn_fwd", c)["W"]
            assert R.worst_ratio(Wm.cpu(), want_W[li], bound) <= TOL.limit("wn_fwd")
        else:
            assert torch.equal(Wm.cpu().double(), want_W[li])


# ======================================================================================================= hoist, colsum, copies
def test_hoist_exact():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for si, (n, c0, o) in enumerate(itertools.product((1, 63, 64, 65, 69), (0, 3, 14), (1, 8, 256))):
        in_dim = c0 + n + 3
        W, b, vec = R.ints((o, in_dim), 6000 + si), R.ints((o,), 6100 + si), R.ints((n,), 6200 + si)
        We, be, ve = _in(W), _in(b), _in(vec)
        b2 = _vec(o, 1)
        L.mp_tr_hoist_fwd(_vp(We.data_ptr()), o, in_dim, _vp(be.data_ptr()), c0, n, _vp(ve.data_ptr()), _vp(b2.data_ptr()), st)
        x = R.NS(W=W.double(), b=b.double(), vec=vec.double(), c0=c0, n=n)
        assert torch.equal(b2.check().cpu().double(), R.ref_hoist_fwd(x)["b2"]), (n, c0, o)
        db2, dW0 = R.ints((o,), 6300 + si), R.ints((o, in_dim), 6400 + si)
        dbe = _in(db2)
        dW = _out(o, in_dim, init=dW0)
        L.mp_tr_hoist_bwd(_vp(dbe.data_ptr()), o, in_dim, c0, n, _vp(ve.data_ptr()), _vp(dW.data_ptr()), st)
        x = R.NS(dW0=dW0.double(), db2=db2.double(), vec=vec.double(), c0=c0, n=n)
        got = dW.check().cpu()
        assert torch.equal(got.double(), R.ref_hoist_bwd(x)["dW"]), (n, c0, o)     # the columns outside c0..c0+n included
        n_run += 1
    assert n_run == 45
    # random floats, per-element bound
    inp = {"W": R.randn((8, 90), 6500), "b": R.randn((8,), 6501), "c0": 14, "n": 69, "vec": R.randn((69,), 6502)}
    We, be, ve = _in(inp["W"]), _in(inp["b"]), _in(inp["vec"])
    b2 = _vec(8)
    L.mp_tr_hoist_fwd(_vp(We.data_ptr()), 8, 90, _vp(be.data_ptr()), 14, 69, _vp(ve.data_ptr()), _vp(b2.data_ptr()), st)
    _check("hoist_fwd", inp, {"b2": b2.check()})
    _report("hoist_fwd")


def test_colsum_exact_and_bounded():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for si, (rows, Cc, ldk) in enumerate(itertools.product((1, 63, 64, 255, 256, 257, 1000), (1, 3, 256), ("C", "C+5", "257"))):
        ld = {"C": Cc, "C+5": Cc + 5, "257": 257}[ldk]
        for kind in ("int", "float"):
            dZ = R.ints((rows, Cc), 7000 + si) if kind == "int" else R.randn((rows, Cc), 7000 + si)
            E = _in(dZ, ld)                                      # the rows past `rows` hold NaN
            db = _vec(Cc, 1)
            L.mp_tr_colsum(_vp(E.data_ptr()), ld, rows, Cc, _vp(db.data_ptr()), st)
            if kind == "int":
                assert torch.equal(db.check().cpu().double(), dZ.double().sum(0)), (rows, Cc, ld)
            else:
                _check("colsum", {"dZ": dZ, "rows": rows}, {"db": db.check()})
            n_run += 1
    assert n_run == 126
    _report("colsum")


def test_copy_cols_exact():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for si, (rows, Cc, c0s, c0d, acc, scale) in enumerate(itertools.product((1, 257), (1, 3, 8), (0, 3), (0, 5), (0, 1), (1.0, RS2))):
        src, dst0 = R.randn((rows, Cc), 7500 + si), R.randn((rows, Cc), 7600 + si)
        S = _in(src, c0s + Cc + 2, c0s)
        D = _out(rows, Cc, c0d + Cc + 1, c0d, init=dst0)
        L.mp_tr_copy_cols(_vp(S.data_ptr() - 4 * c0s), S.ld, c0s, _vp(D.data_ptr() - 4 * c0d), D.ldc, c0d, rows, Cc, scale, acc, st)
        got = D.check().cpu()
        cands = R.copy_cols_candidates(src, scale, dst0, acc)
        ok = torch.zeros_like(got, dtype=torch.bool)
        for c in cands:
            ok |= got == c
        assert bool(ok.all()), (rows, Cc, c0s, c0d, acc, scale)
        n_run += 1
    assert n_run == 96


def test_sigmoid():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    for n in (1, 255, 257, 1000):
        z = R.randn((n,), 7700 + n, 3.0)
        z[0] = 0.0
        if n > 2:
            z[1], z[2] = 30.0, -100.0
        Z, Y = _in(z), _vec(n, 1)
        L.mp_tr_sigmoid_fwd(_vp(Z.data_ptr()), n, _vp(Y.data_ptr()), st)
        y = Y.check()
        _check("sigmoid_fwd", {"Z": z}, {"Y": y})
        dy = R.randn((n,), 7800 + n)
        Ye, dYe, dZ = _in(y.cpu()), _in(dy), _vec(n, 3)
        L.mp_tr_sigmoid_bwd(_vp(Ye.data_ptr()), _vp(dYe.data_ptr()), n, _vp(dZ.data_ptr()), st)
        _check("sigmoid_bwd", {"Y": y.cpu(), "dY": dy}, {"dZ": dZ.check()})
    _report("sigmoid_fwd", "sigmoid_bwd")


# ============================================================================================================ shade_in and eik
def _z8(P, inp, n):
    """Z8 [4P][257]: random features, column 0 = sdf on the value rows and d sdf / dx on the tangent rows"""
    Z8 = R.randn((4 * P, R.Z8_LD), 8000 + P)
    Z8[:n, 0] = inp["sdf"]
    for k in range(3):
        Z8[(k + 1) * P:(k + 1) * P + n, 0] = inp["g"][:, k]
    return Z8


@pytest.mark.parametrize("mode", ("tangent rows", "separate grad"))
def test_shade_in(mode):
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for P, cut, extra, want_djinv in itertools.product((5, 300), (0, 2), (True, False), (True, False)):
        n = P - cut
        inp = R.case_shade(n, 8100 + P + cut, extra)
        xc, jinv = _in(inp["xc"]), _in(inp["jinv"])
        XR, nrm = _out(n, 6), _out(n, 3)
        if mode == "tangent rows":
            Z8h = _z8(P, inp, n)
            Z8 = _in(Z8h)
            sdf = _vec(n, 1)
            L.mp_tr_shade_in_fwd(_vp(Z8.data_ptr()), P, n, _vp(xc.data_ptr()), _vp(jinv.data_ptr()), _vp(XR.data_ptr()),
                                 _vp(nrm.data_ptr()), _vp(sdf.data_ptr()), None, st)
            assert torch.equal(sdf.check().cpu(), inp["sdf"])
        else:
            Z8 = None
            grad = _in(inp["g"])
            L.mp_tr_shade_in_fwd(None, P, n, _vp(xc.data_ptr()), _vp(jinv.data_ptr()), _vp(XR.data_ptr()), _vp(nrm.data_ptr()),
                                 None, _vp(grad.data_ptr()), st)
        xr, nr = XR.check(), nrm.check()
        assert torch.equal(xr[:, :3].cpu(), inp["xc"]) and torch.equal(xr[:, 3:], nr)
        _check("shade_in_fwd", inp, {"nrm": nr})
        assert float(nr[0].abs().max()) == 0.0                     # the zero-gradient point
        # ---- adjoint
        dXR, dsdf = _in(inp["dXR"]), _in(inp["dsdf"])
        dne = _in(inp["dnrm_extra"]) if extra else None
        dj = _out(n, 9) if want_djinv else None
        if mode == "tangent rows":
            fill = R.ints((4 * P, R.Z8_LD), 8200 + P)               # the caller zero-fills; a pattern shows every stray write
            dZ8 = _out(4 * P, R.Z8_LD, init=fill)
            L.mp_tr_shade_in_bwd(_vp(Z8.data_ptr()), P, n, _vp(jinv.data_ptr()), _vp(dXR.data_ptr()), _vp(dsdf.data_ptr()),
                                 _vp(dne.data_ptr()) if extra else None, _vp(dZ8.data_ptr()), _vp(dj.data_ptr()) if dj else None,
                                 None, None, st)
            d8 = dZ8.check().cpu()
            assert torch.equal(d8[:, 1:], fill[:, 1:]), "columns 1..256 of dZ8 changed"
            assert torch.equal(d8[:n, 0], inp["dsdf"])
            dg = torch.stack([d8[(k + 1) * P:(k + 1) * P + n, 0] for k in range(3)], 1)
            for k in range(4):                                    # the points past n_pts of every block
                assert torch.equal(d8[k * P + n:(k + 1) * P, 0], fill[k * P + n:(k + 1) * P, 0])
        else:
            dgr = _out(P, 3, init=R.ints((P, 3), 8300))
            L.mp_tr_shade_in_bwd(None, P, n, _vp(jinv.data_ptr()), _vp(dXR.data_ptr()), _vp(dsdf.data_ptr()),
                                 _vp(dne.data_ptr()) if extra else None, None, _vp(dj.data_ptr()) if dj else None,
                                 _vp(grad.data_ptr()), _vp(dgr.data_ptr()), st)
            full = dgr.check().cpu()
            assert torch.equal(full[n:], R.ints((P, 3), 8300)[n:])
            dg = full[:n]
        ref = R.reference("shade_in_bwd", inp)
        bnd = R.bounds("shade_in_bwd", inp)
        got = {"dg": dg}
        if dj:
            got["djinv"] = dj.check().cpu()
        for k, gv in got.items():
            r = R.worst_ratio(gv, ref[k], bnd[k])
            WORST["shade_in_bwd"] = max(WORST.get("shade_in_bwd", 0.0), r)
            assert r <= TOL.limit("shade_in_bwd"), (k, r)
        assert float(dg[0].abs().max()) > 1e15                     # both clamps active: dn / (1e-6 x 1e-12)
        n_run += 1
    assert n_run == 16
    _report("shade_in_fwd", "shade_in_bwd")


def test_eik_moves():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for P, E in itertools.product((5, 300), (1, 3)):
        e0 = P - E - 1
        assert e0 > 0
        Z8h = R.randn((4 * P, R.Z8_LD), 8400 + P)
        want = torch.stack([Z8h[(k + 1) * P + e0:(k + 1) * P + e0 + E, 0] for k in range(3)], 1)
        Z8 = _in(Z8h)
        gt = _out(E, 3)
        L.mp_tr_eik_fwd(_vp(Z8.data_ptr()), P, e0, E, _vp(gt.data_ptr()), None, st)
        assert torch.equal(gt.check().cpu(), want)
        gradh = R.randn((P, 3), 8500 + P)
        grad = _in(gradh)
        gt = _out(E, 3)
        L.mp_tr_eik_fwd(None, P, e0, E, _vp(gt.data_ptr()), _vp(grad.data_ptr()), st)
        assert torch.equal(gt.check().cpu(), gradh[e0:e0 + E])
        dgt = R.randn((E, 3), 8600 + P)
        dgte = _in(dgt)
        fill = R.ints((4 * P, R.Z8_LD), 8700 + P)
        dZ8 = _out(4 * P, R.Z8_LD, init=fill)
        L.mp_tr_eik_bwd(P, e0, E, _vp(dgte.data_ptr()), _vp(dZ8.data_ptr()), None, st)
        want8 = fill.clone()
        for k in range(3):
            want8[(k + 1) * P + e0:(k + 1) * P + e0 + E, 0] = dgt[:, k]
        assert torch.equal(dZ8.check().cpu(), want8)              # columns 1..256 and every other row bit-unchanged
        fillg = R.ints((P, 3), 8800 + P)
        dgr = _out(P, 3, init=fillg)
        L.mp_tr_eik_bwd(P, e0, E, _vp(dgte.data_ptr()), None, _vp(dgr.data_ptr()), st)
        wantg = fillg.clone()
        wantg[e0:e0 + E] = dgt
        assert torch.equal(dgr.check().cpu(), wantg)
        n_run += 1
    assert n_run == 4


# ============================================================================================== warp, gather, background
def test_warp_bwd():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for n, with_dj in itertools.product((1, 255, 256, 257, 700), (True, False)):
        inp = R.case_warp(n, 9000 + n, with_dj)
        xc, dxc, jinv = _in(inp["xc"]), _in(inp["dxc"]), _in(inp["jinv"])
        dj = _in(inp["djinv"]) if with_dj else None
        skin, tfs = _in(inp["skin_w"]), _in(inp["tfs"])
        npo, nca = _i32(inp["nn_posed"]), _i32(inp["nn_cano"])
        dtfs = _out(R.NJ, 16, init=inp["dtfs0"])
        L.mp_tr_warp_bwd(_vp(xc.data_ptr()), _vp(dxc.data_ptr()), _vp(jinv.data_ptr()), _vp(dj.data_ptr()) if dj else None,
                         _vp(npo.data_ptr()), _vp(nca.data_ptr()), n, _vp(skin.data_ptr()), _vp(tfs.data_ptr()),
                         _vp(dtfs.data_ptr()), st)
        got = dtfs.check()
        assert torch.equal(got[:, 12:].cpu(), inp["dtfs0"][:, 12:]), "entries 12..15 of a transform changed"
        _check("warp_bwd", inp, {"dtfs": got})
        n_run += 1
    assert n_run == 10
    _report("warp_bwd")


def test_gather_bwd_exact():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for n, nv in itertools.product((0, 1, 500), (1, 255, 257)):
        idx = torch.randint(0, max(nv // 2, 1), (n,), generator=torch.Generator().manual_seed(9100 + n + nv))   # repeats; upper half never drawn
        jinv, dxc, dv0 = R.ints((n, 9), 9200 + n), R.ints((n, 3), 9300 + n), R.ints((nv, 3), 9400 + nv)
        ie = _i32(idx) if n else None
        je, de = (_in(jinv), _in(dxc)) if n else (None, None)
        dverts = _out(nv, 3, init=dv0)
        L.mp_tr_gather_bwd(_vp(ie.data_ptr()) if n else None, n, _vp(je.data_ptr()) if n else None,
                           _vp(de.data_ptr()) if n else None, nv, _vp(dverts.data_ptr()), st)
        x = R.NS(idx=idx, jinv=jinv.double(), dxc=dxc.double(), n_verts=nv, dverts0=dv0.double())
        got = dverts.check().cpu()
        assert torch.equal(got.double(), R.ref_gather_bwd(x)["dverts"]), (n, nv)
        never = torch.ones(nv, dtype=torch.bool)
        never[idx] = False
        assert torch.equal(got[never], dv0[never])
        n_run += 1
    assert n_run == 9


def test_bg_comp():
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    n_run = 0
    for NBG, Rr in itertools.product((1, 2, 33), (1, 257)):
        inp = R.case_bg(Rr, NBG, 9500 + NBG + Rr)
        sdf, rgb, zbg, dout = _in(inp["sdf"]), _in(inp["rgb"]), _in(inp["zbg"]), _in(inp["dout"])
        out = _out(Rr, 3)
        L.mp_tr_bg_comp_fwd(_vp(sdf.data_ptr()), _vp(rgb.data_ptr()), _vp(zbg.data_ptr()), Rr, NBG, _vp(out.data_ptr()), st)
        _check("bg_comp_fwd", inp, {"out": out.check()})
        dsdf, drgb = _out(Rr, NBG), _out(Rr, NBG * 3)
        L.mp_tr_bg_comp_bwd(_vp(sdf.data_ptr()), _vp(rgb.data_ptr()), _vp(zbg.data_ptr()), Rr, NBG, _vp(dout.data_ptr()),
                            _vp(dsdf.data_ptr()), _vp(drgb.data_ptr()), st)
        ds = dsdf.check()
        assert bool((ds.cpu()[inp["sdf"] == 0] == 0).all())        # sdf == 0: sign 0
        _check("bg_comp_bwd", inp, {"dsdf": ds, "drgb": drgb.check().reshape(Rr, NBG, 3)})
        n_run += 1
    assert n_run == 6
    _report("bg_comp_fwd", "bg_comp_bwd")


# ================================================================================================================ empty problems
def test_empty_problems_return_zero_without_a_launch():
    """every entry point with an empty problem and NULL data pointers: status 0 (the binding raises on anything else)"""
    hip = _hip()
    L, st = hip.lib(), hip.stream()
    N = None
    calls = [
        lambda: L.mp_tr_pe(N, 3, 0, 6, 1, 1.0, N, 64, 0, st),
        lambda: L.mp_tr_softplus_fwd(N, 8, 0, 8, 0, 1.0, N, 8, 0, st),
        lambda: L.mp_tr_softplus_fwd(N, 8, 4, 0, 0, 1.0, N, 8, 0, st),
        lambda: L.mp_tr_softplus_bwd(N, 8, 0, 8, 0, 1.0, N, 8, 0, N, 8, st),
        lambda: L.mp_tr_relu_bwd(N, 8, 0, 8, N, 8, N, 8, st),
        lambda: L.mp_tr_shade_in_fwd(N, 4, 0, N, N, N, N, N, N, st),
        lambda: L.mp_tr_shade_in_bwd(N, 4, 0, N, N, N, N, N, N, N, N, st),
        lambda: L.mp_tr_eik_fwd(N, 4, 1, 0, N, N, st),
        lambda: L.mp_tr_eik_bwd(4, 1, 0, N, N, N, st),
        lambda: L.mp_tr_sigmoid_fwd(N, 0, N, st),
        lambda: L.mp_tr_sigmoid_bwd(N, N, 0, N, st),
        lambda: L.mp_tr_wn_fwd(N, N, 0, 8, N, N, st),
        lambda: L.mp_tr_wn_bwd(N, N, 0, 8, N, N, N, st),
        lambda: L.mp_tr_wn_fwd_multi(N, 0, 0, st),
        lambda: L.mp_tr_wn_bwd_multi(N, 0, 0, N, N, st),
        lambda: L.mp_tr_hoist_fwd(N, 0, 8, N, 0, 4, N, N, st),
        lambda: L.mp_tr_hoist_bwd(N, 0, 8, 0, 4, N, N, st),
        lambda: L.mp_tr_hoist_bwd(N, 8, 8, 0, 0, N, N, st),
        lambda: L.mp_tr_colsum(N, 8, 4, 0, N, st),
        lambda: L.mp_tr_bg_points(N, N, N, 0, 4, 3.0, N, st),
        lambda: L.mp_tr_bg_points(N, N, N, 4, 0, 3.0, N, st),
        lambda: L.mp_tr_bg_comp_fwd(N, N, N, 0, 4, N, st),
        lambda: L.mp_tr_bg_comp_bwd(N, N, N, 0, 4, N, N, N, st),
        lambda: L.mp_tr_bg_comp_bwd(N, N, N, 4, 0, N, N, N, st),
        lambda: L.mp_tr_pe_bwd(N, 3, 0, 6, 1, N, 64, N, st),
        lambda: L.mp_tr_warp_bwd(N, N, N, N, N, N, 0, N, N, N, st),
        lambda: L.mp_tr_gather_bwd(N, 4, N, N, 0, N, st),
        lambda: L.mp_tr_gather_bwd(N, 0, N, N, 4, N, st),
        lambda: L.mp_tr_sigmul(N, 8, 0, 8, N, 8, N, 1.0, N, 8, st),
        lambda: L.mp_tr_rev_adj(N, 8, 0, 8, N, 8, N, 1.0, N, 8, N, 8, N, 8, st),
        lambda: L.mp_tr_dz(N, 8, 0, 8, N, 8, 1.0, N, 8, N, 8, st),
        lambda: L.mp_tr_dz(N, 8, 4, 0, N, 8, 1.0, N, 8, N, 8, st),
        lambda: L.mp_tr_pe_grad_fwd(N, 0, 6, N, 39, N, st),
        lambda: L.mp_tr_pe_grad_bwd(N, 0, 6, N, N, 39, N, 39, N, st),
        lambda: L.mp_tr_copy_cols(N, 8, 0, N, 8, 0, 0, 8, 1.0, 0, st),
        lambda: L.mp_tr_copy_cols(N, 8, 0, N, 8, 0, 4, 0, 1.0, 0, st),
    ]
    for i, f in enumerate(calls):
        assert f() == 0, i
    torch.cuda.synchronize()
    assert len(calls) == 36
