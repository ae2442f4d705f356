"""The formula behind mp_tf_sdf_dx, pinned against torch autograd in float64 (no GPU): the adjoint of the input points of the
foreground SDF net is J_PE^T (dZ_0 W_0[:, 0:39] + dZ_4 W_4[:, 217:256] / sqrt 2) plus the share that differentiates the
Jacobian of the Fourier features inside d sdf / d x (the one mp_tr_pe_grad_bwd delivers on the device)."""
import math

import torch

from oracle import multiply_oracle as O
from tests.fused_dx_reference import fused_dx_reference
from tests.util import seeded_networks

PREFIX = "foreground_implicit_network_list.0."


def _net64(seed):
    """effective float64 weights (weight norm resolved) of a seeded foreground ImplicitNet, perturbed away from the geometric
    initialisation so that hidden units sit in the softplus transition (sigma'' != 0: the second-order paths carry weight)"""
    m, _ = seeded_networks(1, seed)
    torch.manual_seed(11)
    with torch.no_grad():
        for prm in m.foreground_implicit_network_list[0].parameters():
            prm.add_(torch.randn_like(prm) * 0.02 * prm.abs().mean().clamp_min(1e-2))
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    return [O.linear_params(sd, PREFIX, l) for l in range(9)]


def _forward64(layers, emb, cond):
    """networks.py:160-181 with every pre-activation kept; -> out [P][257], [Z_0 .. Z_8]"""
    h, Z = emb, []
    for l, (w, b) in enumerate(layers):
        if l == 0:
            h = torch.cat([h, cond.view(1, -1).expand(h.shape[0], -1)], -1)
        if l == 4:
            h = torch.cat([h, emb], 1) / math.sqrt(2.0)
        z = torch.nn.functional.linear(h, w, b)
        Z.append(z)
        h = O.softplus100(z) if l < 8 else z
    return h, Z


def test_fused_dx_formula_against_autograd_in_float64():
    layers = _net64(0)
    assert [tuple(w.shape) for w, _ in layers][0] == (256, 108) and tuple(layers[4][0].shape) == (256, 256)
    g = torch.Generator().manual_seed(5)
    P = 97
    x = (torch.rand(P, 3, generator=g, dtype=torch.float64) - 0.5) * 1.6
    cond = torch.randn(69, generator=g, dtype=torch.float64) * 0.1
    a_out = torch.randn(P, 257, generator=g, dtype=torch.float64)
    a_g = torch.randn(P, 3, generator=g, dtype=torch.float64)

    xg = x.clone().requires_grad_(True)
    emb = O.fourier_embed(xg, 6)
    out, Z = _forward64(layers, emb, cond)
    grad = torch.autograd.grad(out[:, 0].sum(), xg, create_graph=True)[0]
    loss = (out * a_out).sum() + (grad * a_g).sum()      # random adjoints on output and gradient (tests/test_train_gpu.py)
    Z[0].retain_grad()      # (only now: the hook would also collect the first-order pass above)
    Z[4].retain_grad()
    loss.backward()
    want = xg.grad
    dZ0, dZ4 = Z[0].grad, Z[4].grad
    assert float(dZ0.abs().max()) > 0 and float(dZ4.abs().max()) > 0

    # autograd's own second-order share: d sdf / d x = J_PE(x)^T G with G = d sdf / d PE; differentiate J_PE alone (G constant)
    G = torch.autograd.grad(_forward64(layers, emb, cond)[0][:, 0].sum(), emb)[0].detach()
    x2 = x.clone().requires_grad_(True)
    grad2 = torch.autograd.grad((O.fourier_embed(x2, 6) * G).sum(), x2, create_graph=True)[0]
    assert torch.allclose(grad2, grad.detach(), rtol=1e-12, atol=1e-14)
    second = torch.autograd.grad((grad2 * a_g).sum(), x2)[0]
    assert float(second.abs().max()) > 1e-3 * float(want.abs().max())      # (both shares matter in this check)

    dx, S = fused_dx_reference(dZ0, dZ4, layers[0][0], layers[4][0], x)
    err = float((dx + second - want).abs().max()) / float(want.abs().max())
    print(f"[fused dx formula] helper + second-order share vs autograd: rel-to-max {err:.3e} (|want|max {float(want.abs().max()):.3e})")
    assert err < 1e-10
    assert bool((S >= dx.abs() * (1 - 1e-12)).all())
    # accumulation onto what is already there
    dx0 = torch.randn(P, 3, generator=g, dtype=torch.float64)
    dx_acc, S_acc = fused_dx_reference(dZ0, dZ4, layers[0][0], layers[4][0], x, dx0)
    assert torch.allclose(dx_acc, dx + dx0, rtol=0, atol=1e-12 * float(dx.abs().max())) and torch.equal(S_acc, S + dx0.abs())
