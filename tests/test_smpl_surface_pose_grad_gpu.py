"""The smpl_surface regulariser (multiply.py:336-362) while the body-model inputs are optimised, opt-in
(model.smpl_surface_pose_grad / MP_SMPL_SURFACE_POSE_GRAD=1): the term reaches smpl_pose / smpl_trans / smpl_shape through the
sampled posed vertices (SMPLServer.pose_backward), their canonical warp (the bone transforms) and the pose conditioning.
Reference: the oracle's training forward under torch autograd, with the surface term restated on top of its pieces so that
the sampled vertices stay attached to the body model (the reference's index_select of smpl_verts, multiply.py:350)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import multiply_oracle as O
from tests.test_train_step_gpu import _cpu, _train_setup, graph_index_in_surface

pytestmark = pytest.mark.gpu

BODY = ("smpl_pose", "smpl_trans", "smpl_shape")
EPOCH = 30                       # both regulariser schedules on, and the pose conditioning (cond_zero off)


def _surface_loss(oracle, inp, draws, vertex_path=True, other_paths=True):
    """multiply.py:336-362 on the oracle's pieces, the sampled vertices NOT detached.  vertex_path / other_paths: keep only the
    gradient through the sampled vertices, or only the one through the transforms and the conditioning."""
    scale = inp["smpl_params"][0, :, 0]
    total = torch.zeros(1)
    for p, dr in draws["person"].items():
        so = oracle.servers[p].forward(scale[p], inp["smpl_trans"][0, p], inp["smpl_pose"][0, p], inp["smpl_shape"][0, p])
        pv, tfs = so["smpl_verts"], so["smpl_tfs"]
        cond = inp["smpl_pose"][0, p, 3:] / np.pi
        if not vertex_path:
            pv = pv.detach()
        if not other_paths:
            tfs, cond = tfs.detach(), cond.detach()
        sample = pv.reshape(-1, 3)[dr["surf_idx"].long()]
        xs, _ = O.deform_inverse(sample, tfs, pv.detach(), oracle.persons[p].server.weights)
        ss = oracle.persons[p].implicit(xs, cond)[:, 0]
        bad = ss > 0.02
        if bool(bad.any()):
            total = total + F.l1_loss(ss[bad], torch.full_like(ss[bad], 0.02), reduction="mean")
    return total


def _setup():
    model, oracle, inp, gin, gt, loss_fn, train = _train_setup()
    model.smpl_surface_weight = loss_fn.smpl_surface_weight = 1.0
    nv = model.smpl_server_list[0].verts_c.reshape(-1, 3).shape[0]
    ids = list(range(nv))
    model.smpl_vertex_part = {"head": ids[:300], "rightHand": ids[300:400], "leftHand": ids[400:500], "rightFoot": ids[500:560],
                              "leftFoot": ids[560:620], "leftHandIndex1": ids[620:640], "rightHandIndex1": ids[640:660]}
    torch.manual_seed(21)
    with torch.no_grad():   # (the geometric initialisation: conditioning columns zero, surface below 0.02 -- perturb both)
        for net in model.foreground_implicit_network_list:
            net.lin0.weight_v[:, 39:] += 0.05 * torch.randn_like(net.lin0.weight_v[:, 39:])
            net.lin8.bias[0] += 0.03
    oracle.sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for pp in oracle.persons:
        pp.sd = oracle.sd
    for k in BODY:
        gin[k] = gin[k].clone().requires_grad_(True)
    gin["smpl_pose_last"] = gin["smpl_pose"].detach() + 0.01
    return model, oracle, inp, gin, gt, loss_fn


def test_smpl_surface_reaches_the_body_model_inputs_when_opted_in():
    model, oracle, inp, gin, gt, loss_fn = _setup()
    model.smpl_surface_pose_grad = True
    R = inp["uv"].shape[1]
    hit = [torch.arange(R), torch.arange(R)]
    out = model({**gin, "hit_index": hit, "current_epoch": EPOCH})
    lo = loss_fn(out, gt)
    lo["loss"].backward()
    torch.cuda.synchronize()
    graph = model._last_train
    assert float(out["smpl_surface_loss"]) > 0
    oin = dict(inp)
    for k in BODY:
        oin[k] = inp[k].clone().requires_grad_(True)
    draws = _cpu(graph.draws)
    z_given = [graph.fg[p]["zfinal"].cpu() for p in range(2)]
    base = {**draws, "person": {p: {k: v for k, v in d.items() if k != "surf_idx"} for p, d in draws["person"].items()}}
    want = oracle.forward_train(oin, hit, z_given, base)            # everything but the surface term
    ssl = _surface_loss(oracle, oin, draws)
    print(f"[parity] smpl_surface_loss: gpu {float(out['smpl_surface_loss']):.6f} oracle {float(ssl):.6f}")
    assert abs(float(out["smpl_surface_loss"]) - float(ssl)) < 2e-5 * max(1.0, abs(float(ssl)))
    want.update(fg_rgb_values_each_person_list=[], index_in_surface=graph_index_in_surface(out), epoch=EPOCH,
                temporal_loss=torch.zeros(1), smpl_surface_loss=ssl, zero_pose_loss=torch.zeros(1),
                sam_mask=gin["sam_mask"].squeeze().cpu())
    lw = loss_fn(want, gt)
    assert abs(float(lo["loss"]) - float(lw["loss"])) < 3e-4 * max(1.0, abs(float(lw["loss"])))
    g_all = torch.autograd.grad(lw["loss"], [oin[k] for k in BODY], retain_graph=True)
    g_vert = torch.autograd.grad(_surface_loss(oracle, oin, draws, other_paths=False).sum(), [oin[k] for k in BODY])
    g_surf = torch.autograd.grad(_surface_loss(oracle, oin, draws).sum(), [oin[k] for k in BODY])
    for k, ga, gv, gs in zip(BODY, g_all, g_vert, g_surf):
        a = gin[k].grad.cpu()
        m = ga.abs().max().item() + 1e-12
        e = (a - ga).abs().max().item() / m
        share_v, share_s = gv.abs().max().item() / m, gs.abs().max().item() / m
        print(f"[grad parity] d loss / d {k} with smpl_surface (opt-in): rel-to-max err {e:.3e}; the term's share {share_s:.2e}, "
              f"its vertex path's {share_v:.2e}")
        assert e < 2e-4, k                                          # measured 7e-6 .. 2.2e-5 (backward row)
        # the vertex path must be well above the error, or its absence would pass unnoticed.  (The whole term's share of d transl
        # is ~0: a translation moves the sampled vertices and the transforms together, and x_c does not move.)
        assert share_v > 5 * e, k
        if k == "smpl_pose":
            assert share_s > 5 * e, k


def test_smpl_surface_under_pose_optimisation_still_refuses_by_default():
    model, oracle, inp, gin, gt, loss_fn = _setup()
    if os.environ.get("MP_SMPL_SURFACE_POSE_GRAD") is None:
        assert model.smpl_surface_pose_grad is False                 # the default
    model.smpl_surface_pose_grad = False
    R = inp["uv"].shape[1]
    with pytest.raises(NotImplementedError):
        model({**gin, "hit_index": [torch.arange(R), torch.arange(R)], "current_epoch": EPOCH})
