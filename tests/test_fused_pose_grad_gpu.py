"""Pose optimisation on the layer-fused SDF training kernels: mp_tf_sdf_dx (csrc/tfuse.hip), the adjoint of the input points
from the stash mp_tf_sdf_bwd leaves behind -- the kernel alone against its float64 restatement, ImplicitTrainFused's
backward(want_dx=True) against torch autograd and the layer-wise evaluator, and the training step with the body-model inputs
under optimisation in both SDF_POSE_GRAD_MODEs against the oracle."""
import pytest
import torch

from oracle import multiply_oracle as O
from tests.fused_dx_reference import fused_dx_reference
from tests.test_train_gpu import _implicit_torch, rel
from tests.util import seeded_networks

pytestmark = pytest.mark.gpu

TILE = 128            # points per workgroup tile of k_tf_sdf_dx (16 per wave); a workgroup walks tiles with a stride of 256
MAX_GRID = 256


def _kernel_case(P, seed):
    """random stashes dZ_0 / dZ_4 inside the first five [P+1][256] tensors of an arena (the part mp_tf_sdf_dx reads), their pad
    rows NaN; random weights; x in +-0.8; random dx to accumulate onto"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    R1 = 256 * (P + 1)
    arena = torch.randn(5 * R1, device="cuda", generator=g)
    t = arena.view(5, P + 1, 256)
    t[0, P] = float("nan")
    t[4, P] = float("nan")
    W0 = torch.randn(256, 108, device="cuda", generator=g)
    W4 = torch.randn(256, 256, device="cuda", generator=g)
    x = (torch.rand(P, 3, device="cuda", generator=g) - 0.5) * 1.6
    dx0 = torch.randn(P, 3, device="cuda", generator=g)
    return arena, t, W0, W4, x, dx0


# one point; less than a wave; around a wave boundary (64 = 4 x 16) and around a tile boundary; five full tiles and a ragged one;
# 258 tiles: the first two workgroups walk a second tile (the one whose rows they prefetch), the other 254 do not
@pytest.mark.parametrize("P", [1, 5, 63, 64, 65, 127, 128, 129, 700, MAX_GRID * TILE + TILE + 1])
def test_sdf_dx_kernel_against_float64(P):
    """|got - want| <= 600 * 2^-24 * S per component, S = the sum of the absolute values of all terms: the worst case of a
    512-term fp32 chain plus the 26 Fourier terms, with headroom for the trigonometric functions, in ANY order of summation --
    an indexing error shows as O(S)."""
    from multiply_amd import hip
    L, st = hip.lib(), hip.stream()
    arena, t, W0, W4, x, dx0 = _kernel_case(P, 100 + P % 97)
    dx = dx0.clone()
    L.mp_tf_sdf_dx(arena, P, W0, 108, W4, 256, x, dx, st)
    torch.cuda.synchronize()
    want, S = fused_dx_reference(t[0, :P], t[4, :P], W0, W4, x, dx0)
    got = dx.double().cpu()
    assert bool(torch.isfinite(got).all())
    ratio = ((got - want).abs() / (2.0 ** -24 * S)).max().item()
    print(f"[sdf dx kernel] P {P}: max |got - want| = {ratio:.2f} x 2^-24 S  (bound 600; |want|max {want.abs().max().item():.3e})")
    assert ratio <= 600.0
    assert not torch.equal(dx, dx0)
    dx2 = dx0.clone()
    L.mp_tf_sdf_dx(arena, P, W0, 108, W4, 256, x, dx2, st)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx)                       # fixed summation order: bit-identical from launch to launch


def test_sdf_dx_kernel_without_points_does_nothing():
    from multiply_amd import hip
    arena, t, W0, W4, x, dx0 = _kernel_case(5, 3)
    dx = dx0.clone()
    assert hip.lib().mp_tf_sdf_dx(arena, 0, W0, 108, W4, 256, x, dx, hip.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0)


def test_sdf_dx_kernel_refuses_weight_rows_without_the_fourier_columns():
    """ldw0 < 39 or ldw4 < 256: status -1 (the binding raises with the entry point's name), nothing launched"""
    from multiply_amd import hip
    arena, t, W0, W4, x, dx0 = _kernel_case(5, 4)
    dx = dx0.clone()
    for ldw0, ldw4 in ((38, 256), (108, 255)):
        with pytest.raises(RuntimeError, match="mp_tf_sdf_dx failed with code -1"):
            hip.lib().mp_tf_sdf_dx(arena, 5, W0, ldw0, W4, ldw4, x, dx, hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0)


@pytest.mark.parametrize("P", [700, 129, 5])
def test_fused_evaluator_yields_the_adjoint_of_the_points(P, monkeypatch):
    """ImplicitTrainFused.backward(want_dx=True) against torch autograd with create_graph on the oracle's formula (rel < 5e-4) and
    against the layer-wise evaluator on exact-fp32 GEMMs (rel < 2e-4): the bounds tests/test_train_gpu.py holds the fused
    PARAMETER gradients to, which are contractions of the same dZ_l.  The weights are the perturbed ones of
    test_fused_sdf_kernels_against_autograd (sigma'' != 0).  The parameter gradients and d cond do not depend on want_dx."""
    from multiply_amd import train as T
    monkeypatch.setattr(T, "TRAIN_PRECISION", "f32")            # (the layer-wise reference's GEMMs, as in tests/test_train_gpu.py)
    m, _ = seeded_networks(1, 0)
    m = m.cuda()
    net = m.foreground_implicit_network_list[0]
    torch.manual_seed(11)
    with torch.no_grad():
        for prm in net.parameters():
            prm.add_(torch.randn_like(prm) * 0.02 * prm.abs().mean().clamp_min(1e-2))
    assert T.fused_sdf_supported(net)
    x = (torch.rand(P, 3, device="cuda") - 0.5) * 1.6
    cond = torch.randn(69, device="cuda") * 0.1
    a_out = torch.randn(P, 257, device="cuda")
    a_g = torch.randn(P, 3, device="cuda")
    # reference 1: autograd
    sd = {k: v for k, v in m.named_parameters()}
    xg = x.clone().requires_grad_(True)
    out = O.implicit_forward(sd, "foreground_implicit_network_list.0.", xg, cond, 6)
    g = torch.autograd.grad(out[:, 0].sum(), xg, create_graph=True)[0]
    loss = (out * a_out).sum() + (g * a_g).sum()
    (want,) = torch.autograd.grad(loss, xg)
    # reference 2: the layer-wise evaluator
    ref = T.ImplicitTrainRev(net, x, cond)
    ref.backward(a_out.clone(), None, a_g.clone(), want_dx=True)
    fus = T.ImplicitTrainFused(net, x, cond)
    dc1 = fus.backward(a_out[:, 1:].contiguous(), a_out[:, 0].contiguous(), a_g.clone(), want_dx=True).clone()
    assert fus.dx.shape == (P, 3)
    dx = fus.dx.clone()
    grads1 = [t.clone() for t in fus.param_grads()]
    e_ref = rel("layer-wise d x vs autograd", ref.dx, want)
    e_fus = rel("fused d x vs autograd", dx, want)
    e_lw = rel("fused d x vs layer-wise", dx, ref.dx)
    # (the layer-wise path itself beyond 5e-4 on these inputs: the fused one is held to twice its error)
    assert e_fus < (5e-4 if e_ref <= 5e-4 else 2 * e_ref)
    assert e_lw < 2e-4
    # a fresh evaluator without want_dx: the same launches as before the points' adjoint existed
    fus2 = T.ImplicitTrainFused(net, x, cond)
    dc2 = fus2.backward(a_out[:, 1:].contiguous(), a_out[:, 0].contiguous(), a_g.clone())
    assert fus2.dx is None
    assert rel("d cond, want_dx or not", dc1, dc2) < 1e-5
    grads2 = fus2.param_grads()
    assert len(grads1) == len(grads2) > 0
    for i, (g1, g2) in enumerate(zip(grads1, grads2)):
        assert rel(f"parameter gradient {i}, want_dx or not", g1, g2) < 1e-5


def test_training_step_with_body_inputs_under_optimisation_in_both_modes(monkeypatch):
    """11 x 11 rays, 2 persons, all rays hit, smpl_pose / smpl_trans / smpl_shape with requires_grad, ONE set of draws: the step
    in SDF_POSE_GRAD_MODE 'layerwise' (ImplicitTrainRev) and 'fused' (ImplicitTrainFused + mp_tf_sdf_dx), both against the
    oracle under torch autograd with the bounds of test_training_gradients_to_body_model_params, the network parameter gradients
    of the two against each other with the bound of test_forward_mode_and_reverse_mode_training_agree."""
    from multiply_amd import train as T
    from tests.test_train_step_gpu import _cpu, _train_setup
    model, oracle, inp, gin, gt, loss_fn, train = _train_setup()
    R = inp["uv"].shape[1]
    hit = [torch.arange(R), torch.arange(R)]
    body = ("smpl_pose", "smpl_trans", "smpl_shape")
    for k in body:
        gin[k] = gin[k].clone().requires_grad_(True)
    gin["smpl_pose_last"] = gin["smpl_pose"].detach() + 0.01
    assert T.SDF_TRAIN_MODE == "fused" and T.TRAIN_PRECISION == "bf16x3"
    res, draws, z_given = {}, None, None
    for mode in ("layerwise", "fused"):
        monkeypatch.setattr(T, "SDF_POSE_GRAD_MODE", mode)
        if draws is None:
            cx = model._setup({**gin, "hit_index": hit}, -1, False)
            draws = T.make_draws(model, cx, None)
        out = T.forward_train(model, {**gin, "hit_index": hit}, draws=draws)
        lo = loss_fn(out, gt)
        model.zero_grad()
        for k in body:
            gin[k].grad = None
        lo["loss"].backward()
        torch.cuda.synchronize()
        graph = model._last_train
        assert graph.pose_grad
        for p in range(2):
            it = graph.fg[p]["it"]
            assert isinstance(it, T.ImplicitTrainFused if mode == "fused" else T.ImplicitTrainRev), (mode, type(it))
            assert float(it.dx.abs().max()) > 0
        if z_given is None:
            z_given = [graph.fg[p]["zfinal"].cpu() for p in range(2)]
        res[mode] = (float(lo["loss"]), {k: gin[k].grad.detach().cpu().clone() for k in body},
                     {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    # the oracle, once
    oin = dict(inp)
    for k in body:
        oin[k] = inp[k].clone().requires_grad_(True)
    want = oracle.forward_train(oin, hit, z_given, _cpu(draws))
    tl = torch.mean(torch.square(inp["smpl_pose"] + 0.01 - oin["smpl_pose"]))
    want.update(fg_rgb_values_each_person_list=[], index_in_surface=None, epoch=301, temporal_loss=tl,
                smpl_surface_loss=torch.zeros(1), zero_pose_loss=torch.zeros(1), sam_mask=gin["sam_mask"].squeeze().cpu())
    lw = loss_fn(want, gt)
    gw = torch.autograd.grad(lw["loss"], [oin[k] for k in body])
    for mode in ("layerwise", "fused"):
        loss, gb, _ = res[mode]
        print(f"[pose grad] {mode}: loss {loss:.7f} (oracle {float(lw['loss']):.7f})")
        assert abs(loss - float(lw["loss"])) < 1e-4, mode
        for k, w in zip(body, gw):
            e = (gb[k] - w).abs().max().item() / (w.abs().max().item() + 1e-12)
            print(f"[pose grad] {mode}: d loss / d {k}: rel-to-max err {e:.3e} (|want|max {w.abs().max().item():.3e})")
            assert e < 5e-3, (mode, k)
    for k in body:
        a, b = res["fused"][1][k], res["layerwise"][1][k]
        print(f"[pose grad] fused vs layer-wise d loss / d {k}: rel-to-max {(a - b).abs().max().item() / (b.abs().max().item() + 1e-12):.3e}")
    worst = 0.0
    assert res["fused"][2].keys() == res["layerwise"][2].keys()
    for k, gl in res["layerwise"][2].items():
        gf = res["fused"][2][k]
        r = float((gf - gl).norm() / (gl.norm() + 1e-12))
        worst = max(worst, r)
        assert r < 2e-3 or float((gf - gl).abs().max()) < 1e-7, k
    print(f"[pose grad] fused vs layer-wise network parameter gradients: worst relative difference {worst:.3e}")
