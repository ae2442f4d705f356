"""The float64 references and bounds of tests/train_elementwise_reference.py checked on their own (no GPU): against torch's own
modules and autograd, against the oracle's embedder, against the recorded CPU ratios, and against planted errors."""
import math

import pytest
import torch

from oracle import multiply_oracle as O
from tests import tolerances_train_elementwise as TOL
from tests import train_elementwise_reference as R


def _close(a, b, rtol=1e-12, atol=1e-14):
    return torch.allclose(a, b, rtol=rtol, atol=atol)


def test_softplus_reference_is_torch_softplus_and_its_derivatives():
    z = torch.cat([0.3 * torch.randn(500, generator=torch.Generator().manual_seed(1), dtype=torch.float64),
                   torch.tensor(R.softplus_values(), dtype=torch.float64)])
    z = z[(100.0 * z - 20.0).abs() > 1e-3]                         # away from the branch point
    hi = R.softplus_hi(z.float())
    assert bool((hi == (100.0 * z > 20.0)).all())
    zl = z.clone().requires_grad_(True)
    s, s1, s2 = R.r_s012(zl, hi)
    zt = z.clone().requires_grad_(True)
    t = torch.nn.Softplus(beta=100, threshold=20)(zt)
    t1, = torch.autograd.grad(t.sum(), zt, create_graph=True)
    t2, = torch.autograd.grad(t1.sum(), zt)
    assert _close(s, t) and _close(s1, t1) and _close(s2, t2, atol=1e-12)
    lo, up, z02 = R.branch_floats()
    assert not bool(R.softplus_hi(torch.tensor([lo]))) and bool(R.softplus_hi(torch.tensor([up])))
    assert lo <= z02 <= up and torch.tensor(up).float().item() == up


def test_forward_mode_layer_adjoint_is_a_double_backward():
    """tiny net h = softplus(x W^T): value rows Z0 = x W^T, tangent rows Z_k = W[:, k]; a loss on h and on d h / d x_k,
    differentiated w.r.t. W through torch's create_graph, equals the layer adjoint pulled back through the same linear map"""
    g = torch.Generator().manual_seed(2)
    P, Cc = 6, 4
    x = torch.randn(P, 3, generator=g, dtype=torch.float64)
    W = (0.1 * torch.randn(Cc, 3, generator=g, dtype=torch.float64)).float().double()
    A = torch.randn(4 * P, Cc, generator=g, dtype=torch.float64)
    Wl = W.clone().requires_grad_(True)
    xl = x.clone().requires_grad_(True)
    h = torch.nn.Softplus(beta=100, threshold=20)(xl @ Wl.T)
    cols = [torch.autograd.grad(h[:, c].sum(), xl, create_graph=True)[0] for c in range(Cc)]       # [P][3] each
    tang = [torch.stack([cols[c][:, k] for c in range(Cc)], 1) for k in range(3)]
    loss = (torch.cat([h] + tang, 0) * A).sum()
    dW_true, = torch.autograd.grad(loss, Wl)
    Z = torch.cat([x @ W.T] + [W[:, k].unsqueeze(0).expand(P, Cc) for k in range(3)], 0)
    xns = R.NS(Z=Z, hi=R.softplus_hi(Z.float()), P=P, scale=1.0, dH=A)
    dZ = R.ref_softplus_bwd(xns)["dZ"]
    dW = dZ[:P].T @ x + torch.stack([dZ[(k + 1) * P:(k + 2) * P].sum(0) for k in range(3)], 1)
    assert _close(dW, dW_true, rtol=1e-10, atol=1e-12)
    Hf = R.ref_softplus_fwd(xns)["H"]
    assert _close(Hf, torch.cat([h] + tang, 0).detach(), rtol=1e-10, atol=1e-12)


def test_rev_chain_reference_is_dz_of_rev_adj():
    inp = R.case_rev(16, 8, 3)
    dS = R.reference("rev_adj", inp)["dS"]
    x = R._conv(inp, lambda t: t.double())
    x.dS, x.scale = dS, inp["scale"]
    assert _close(R.ref_dz(x)["dZ"], R.reference("rev_chain", inp)["dZ"], rtol=1e-11, atol=1e-13)


@pytest.mark.parametrize("D,L", [(3, 0), (3, 6), (4, 10)])
def test_pe_layout_is_the_oracle_embedder(D, L):
    x = R.pe_points(9, D, 4).double()
    assert torch.equal(R.pe_ref(x, L), O.fourier_embed(x, L))
    assert R.pe_ref(x, L).shape[1] == R.pe_width(D, L)
    inp = R.case_pe(9, D, L, 0, 1.0, 4)
    assert _close(R.reference("pe", inp)["out"], O.fourier_embed(inp["x"].double(), L))


def test_weight_norm_reference_is_torch_weight_norm():
    c = R.case_wn(5, 7, 5)
    lin = torch.nn.Linear(7, 5, bias=False).double()
    lin = torch.nn.utils.weight_norm(lin)
    with torch.no_grad():
        lin.weight_v.copy_(c["v"].double())
        lin.weight_g.copy_(c["g"].double().view(5, 1))
    eye = torch.eye(7, dtype=torch.float64)
    Wt = lin(eye).T                                                # the effective weight
    assert _close(R.reference("wn_fwd", c)["W"], Wt.detach())
    assert _close(R.reference("wn_fwd", c)["W"], O.weight_norm_effective(c["g"].double().view(5, 1), c["v"].double()))
    (Wt * c["dW"].double()).sum().backward()
    ref = R.reference("wn_bwd", c)
    assert _close(ref["dv"], lin.weight_v.grad) and _close(ref["dg"], lin.weight_g.grad.view(-1))


def test_recorded_cpu_ratios_are_reproduced():
    now = R.cpu_ratios()
    assert set(now) == set(TOL.CPU_RATIO) == set(R.BOUNDED)
    for k, r in now.items():
        assert abs(r - TOL.CPU_RATIO[k]) <= 0.1 * TOL.CPU_RATIO[k], (k, r, TOL.CPU_RATIO[k])
        assert TOL.limit(k) >= 2.0 and r <= TOL.limit(k)


def _rejects(kernel, good, planted_ref, bound):
    """at its limit the bound passes the float32 evaluation of the right tree and rejects the planted reference"""
    return R.worst_ratio(good, planted_ref, bound) > TOL.limit(kernel)


def test_bounds_reject_planted_errors():
    # the sigma'' term dropped from the forward-mode adjoint
    inp = R.case_softplus(20, 8, 5, 4, 1 / math.sqrt(2))
    good, bnd = R.emulate("softplus_bwd", inp)["dZ"], R.bounds("softplus_bwd", inp)["dZ"]
    assert R.worst_ratio(good, R.reference("softplus_bwd", inp)["dZ"], bnd) <= TOL.limit("softplus_bwd")
    assert _rejects("softplus_bwd", good, R.reference("softplus_bwd", inp, drop_d2=True)["dZ"], bnd)
    # a tangent row taken from the wrong block
    x = R._conv(inp, lambda t: t.double())
    good, bnd = R.emulate("softplus_fwd", inp)["H"], R.bounds("softplus_fwd", inp)["H"]
    assert R.worst_ratio(good, R.reference("softplus_fwd", inp)["H"], bnd) <= TOL.limit("softplus_fwd")
    assert _rejects("softplus_fwd", good, R.r_softplus_layer(x.Z, x.hi, x.P, x.scale, wrong_block=True), bnd)
    # one descriptor's row0 off by one
    shapes = [(1, 1), (3, 39), (8, 63), (1, 1)]
    cases = [R.case_wn(o, i, 30 + li) for li, (o, i) in enumerate(shapes)]
    row0, total = R.wn_layout(shapes, [True] * 4, 1)[:2]
    layers = [(c["v"], c["g"]) for c in cases]
    right = R.ref_wn_fwd_multi(layers, row0, total)
    for li, c in enumerate(cases):
        assert _close(right[li], R.reference("wn_fwd", c)["W"])
    wrong = R.ref_wn_fwd_multi(layers, [row0[0], row0[1], row0[2] + 1, row0[3]], total)
    good, bnd = R.emulate("wn_fwd", cases[2])["W"], R.bounds("wn_fwd", cases[2])["W"]
    assert R.worst_ratio(good, right[2], bnd) <= TOL.limit("wn_fwd")
    assert _rejects("wn_fwd", good, wrong[2], bnd)
    # a column sum missing its last row
    inp = {"dZ": R.randn((257, 3), 40), "rows": 257}
    good, bnd = R.emulate("colsum", inp)["db"], R.bounds("colsum", inp)["db"]
    x = R._conv(inp, lambda t: t.double())
    assert R.worst_ratio(good, R.ref_colsum(x)["db"], bnd) <= TOL.limit("colsum")
    assert _rejects("colsum", good, R.ref_colsum(x, drop_last=True)["db"], bnd)


def test_exact_references_and_candidates():
    src, dst = R.randn((5, 3), 50), R.randn((5, 3), 51)
    assert len(R.copy_cols_candidates(src, R.f32(0.7), dst, 1)) == 2 and len(R.copy_cols_candidates(src, 1.0, dst, 0)) == 1
    assert torch.equal(R.copy_cols_candidates(src, 1.0, dst, 0)[0], src)
    idx = torch.tensor([0, 2, 0])
    x = R.NS(idx=idx, jinv=R.ints((3, 9), 52).double(), dxc=R.ints((3, 3), 53).double(), n_verts=4, dverts0=R.ints((4, 3), 54).double())
    want = x.dverts0.clone()
    for s in range(3):
        want[idx[s]] += x.jinv[s].view(3, 3).T @ x.dxc[s]
    assert torch.equal(R.ref_gather_bwd(x)["dverts"], want)
    for row, (li, r) in zip((0, 1, 3, 4, 12), ((0, 0), (1, 0), (1, 2), (2, 0), (3, 0))):
        assert R.wn_find([0, 1, 4, 12], row) == (li, r)
