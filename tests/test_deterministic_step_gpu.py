"""The deterministic training mode on a whole step and on a resumed run (multiply_amd/train.py: model.train_deterministic).

The step is the 121-ray, 2-person step of tests/test_train_step_gpu.py with smpl_pose / smpl_trans / smpl_shape under optimisation:
two forwards and backwards from the same state give the same bits -- loss, the whole flat gradient buffer, the three body-input
gradients -- in both MP_SDF_POSE_GRAD_MODE values and both GEMM precisions, also after the contractions' workspace has moved; against
the default mode the gradients agree within the bounds the existing step tests hold against the oracle.  The opt-in terms
(train_geometry, train_interpenetration, smpl_surface under pose optimisation) pass the same check; person-sharded training raises.

The run: 4 epochs of a written 2-frame scene uninterrupted, against 2 epochs + checkpoint + a fresh Trainer + 2 more epochs: every
parameter, both optimiser states and the body tables are torch.equal."""
import os

import pytest
import torch

from tests import tolerances as TOL
from tests.test_train_step_gpu import _train_setup

pytestmark = pytest.mark.gpu

BODY = ("smpl_pose", "smpl_trans", "smpl_shape")
BODY_REL = 5e-3          # tests/test_train_step_gpu.py::test_training_gradients_to_body_model_params: relative to the maximum


@pytest.fixture(scope="module")
def scene():
    model, oracle, inp, gin, gt, loss_fn, train = _train_setup()
    for k in BODY:
        gin[k] = gin[k].clone().requires_grad_(True)
    gin["smpl_pose_last"] = gin["smpl_pose"].detach() + 0.01
    R = inp["uv"].shape[1]
    assert R == 121
    yield model, gin, gt, loss_fn, [torch.arange(R), torch.arange(R)]
    model.train_deterministic = None


def _flat_gradients(ts):
    """TrainState's flat parameter-gradient buffer where it is written: d v and d g of the weight-normed layers (a layer without
    weight norm hands out its accumulators, compared through the named gradients; the up to three floats of padding behind a
    tensor are never written).  Everything else is zeroed here."""
    live = torch.zeros(ts.grad_size, dtype=torch.bool, device=ts.gbuf.device)
    n = 0
    for ls in ts.lins.values():
        for lp in ls:
            if lp.wn:
                _, _, o_dv, o_dg = ts.layout[id(lp)]
                live[o_dv:o_dv + lp.out_dim * lp.in_dim] = True
                live[o_dg:o_dg + lp.out_dim] = True
                n += 1
    assert n >= 18 and int(live.sum()) > 1_000_000          # the two persons' SDF nets at the least
    return torch.where(live, ts.gbuf, torch.zeros_like(ts.gbuf))


def _step(model, gin, gt, loss_fn, hit, det, extra=None, epoch=None):
    """one forward + backward from the same state and the same seed -> loss, flat gradient buffer, body gradients, named gradients"""
    model.train_deterministic = det
    model.zero_grad(set_to_none=True)
    for k in BODY:
        gin[k].grad = None
    torch.manual_seed(77)                       # the step's draws (train.make_draws)
    inp = {**gin, "hit_index": hit}
    if epoch is not None:
        inp["current_epoch"] = epoch
    out = model(inp)
    lo = loss_fn(out, gt)
    loss = lo["loss"] if extra is None else lo["loss"] + extra(out)
    loss.backward()
    torch.cuda.synchronize()
    graph = model._last_train
    assert graph.pose_grad and graph.det == bool(det)
    return dict(loss=loss.detach().clone(), gbuf=_flat_gradients(graph.ts), body=[gin[k].grad.clone() for k in BODY],
                ssl=float(out["smpl_surface_loss"]),
                named={k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})


def _same(a, b, what):
    assert torch.equal(a["loss"], b["loss"]), (what, "loss")
    assert torch.equal(a["gbuf"], b["gbuf"]), (what, "flat gradient buffer", int((a["gbuf"] != b["gbuf"]).sum()))
    for k, x, y in zip(BODY, a["body"], b["body"]):
        assert torch.equal(x, y), (what, k)
    assert a["named"].keys() == b["named"].keys() and all(torch.equal(a["named"][k], b["named"][k]) for k in a["named"]), (what, "parameters")


def _close_to_default(d, ref, what):
    """the bounds of tests/test_train_step_gpu.py (there: device against oracle): relative L2 error per parameter tensor, relative
    to the maximum for the body inputs"""
    assert abs(float(d["loss"]) - float(ref["loss"])) < 1e-4 * max(1.0, abs(float(ref["loss"])))
    worst = 0.0
    for k, g in ref["named"].items():
        a, b = d["named"][k].double().reshape(-1), g.double().reshape(-1)
        rel = float((a - b).norm() / (b.norm() + 1e-12))
        worst = max(worst, rel)
        tol = TOL.TRAIN_GRAD_REL_RENDERING if "rendering" in k else TOL.TRAIN_GRAD_REL
        assert rel < tol or float((a - b).abs().max()) < 1e-7, (what, k, rel)
    for k, x, y in zip(BODY, d["body"], ref["body"]):
        e = float((x - y).abs().max() / (y.abs().max() + 1e-12))
        worst = max(worst, e)
        assert e < BODY_REL, (what, k, e)
    print(f"[deterministic step] {what}: worst relative difference to the default mode {worst:.3e}")


@pytest.mark.parametrize("precision", ["bf16x3", "f32"])
@pytest.mark.parametrize("pose_mode", ["layerwise", "fused"])
def test_step_is_a_function_of_its_inputs(scene, pose_mode, precision, monkeypatch):
    from multiply_amd import train as T
    monkeypatch.setattr(T, "SDF_POSE_GRAD_MODE", pose_mode)
    monkeypatch.setattr(T, "TRAIN_PRECISION", precision)
    a = _step(*scene, det=True)
    b = _step(*scene, det=True)
    _same(a, b, (pose_mode, precision))
    evaluators = {type(f["it"]).__name__ for f in scene[0]._last_train.fg.values()}
    # (the fused kernels are split-bf16: with the exact-fp32 GEMMs both modes take the layer-wise evaluator)
    assert evaluators == ({"ImplicitTrainFused"} if (pose_mode, precision) == ("fused", "bf16x3") else {"ImplicitTrainRev"})
    if pose_mode == "fused":                    # an unrelated allocation takes the workspace's place: the address must not matter
        assert T.det_workspace_bytes() > 0
        old = {ws.data_ptr() for ws in T._DET_WS.values()}
        T.release_det_workspace()
        squat = torch.empty(T.DET_WS_BYTES // 4 + 4, device="cuda")
        c = _step(*scene, det=True)
        assert {ws.data_ptr() for ws in T._DET_WS.values()} != old and squat is not None
        _same(a, c, (pose_mode, precision, "moved workspace"))
    _close_to_default(a, _step(*scene, det=False), (pose_mode, precision))


GEOMETRY_OUT = ("depth_values", "depth_person_list", "acc_person_solo_list", "depth_person_solo_list", "depth_person_solo_level_list")


@pytest.mark.parametrize("term", ["train_geometry", "train_interpenetration"])
def test_opt_in_terms_are_deterministic(scene, term, monkeypatch):
    from multiply_amd import train as T
    monkeypatch.setattr(T, "SDF_POSE_GRAD_MODE", "fused")
    model = scene[0]
    if term == "train_geometry":
        extra = lambda out: sum(out[k].sum() for k in GEOMETRY_OUT)
    else:
        extra = lambda out: out["interpenetration_loss"].sum()
    setattr(model, term, True)
    try:
        a = _step(*scene, det=True, extra=extra)
        b = _step(*scene, det=True, extra=extra)
        _same(a, b, term)
        _close_to_default(a, _step(*scene, det=False, extra=extra), term)
    finally:
        setattr(model, term, False)


def test_smpl_surface_under_pose_optimisation_is_deterministic():
    from tests.test_smpl_surface_pose_grad_gpu import EPOCH, _setup
    model, oracle, inp, gin, gt, loss_fn = _setup()
    model.smpl_surface_pose_grad = True
    R = inp["uv"].shape[1]
    args = (model, gin, gt, loss_fn, [torch.arange(R), torch.arange(R)])
    a = _step(*args, det=True, epoch=EPOCH)
    assert a["ssl"] > 0
    b = _step(*args, det=True, epoch=EPOCH)
    _same(a, b, "smpl_surface")
    _close_to_default(a, _step(*args, det=False, epoch=EPOCH), "smpl_surface")


def test_person_sharded_training_raises_under_the_flag(scene):
    from multiply_amd import train as T
    model, gin, gt, loss_fn, hit = scene
    model.train_deterministic = True
    try:
        with pytest.raises(NotImplementedError, match="person-sharded"):
            T.forward_train(model, {**gin, "hit_index": hit}, shard=(2, 0))
    finally:
        model.train_deterministic = None


# ========================================================================================================================= resume
def test_resumed_run_equals_the_uninterrupted_run_bit_for_bit(tmp_path):
    """epochs 0 .. 3 of a 2-frame, 2-person scene (two steps per epoch; the plan of every step: joint optimiser, no mesh-space
    term, no SAM stage; mesh refresh, mask refresh and validation configured out by their periods)"""
    from multiply_amd import trainer as TR
    from multiply_amd.synthetic import write_sequence
    from tests.test_trainer_gpu import _build, _final_state
    seq = os.path.join(str(tmp_path), "seq")
    write_sequence(seq, n_frames=2, H=64, W=64, num_person=2)
    cfg = dict(mesh_refresh_period=10 ** 6, mask_refresh_period=10 ** 6, validation_period=10 ** 6, checkpoint_period=10 ** 6,
               deterministic=True)
    for e in range(4):
        plan = TR.step_plan(e, dict(TR.SCHEDULE_DEFAULTS, pose_correction_epoch=500), False, True)
        assert plan["optimizer"] == "joint" and not plan["mesh_losses"] and not plan["freeze_shape"]
    full = _build(tmp_path, "full", seq=seq, seed=3, **cfg)
    full.validset = None
    assert full.model.train_deterministic is True
    full.fit(4)
    want = _final_state(full) + [v.detach().clone() for bm in full.body for v in bm.state_dict().values()]
    a1 = _build(tmp_path, "A", seq=seq, seed=3, **cfg)
    a1.validset = None
    a1.fit(2)
    path = a1.save_checkpoint(os.path.join(a1.out_dir, "checkpoints", "epoch=0001-loss=x.ckpt"))
    assert torch.load(path, map_location="cpu", weights_only=False)["deterministic"] is True
    a2 = _build(tmp_path, "A", seq=seq, seed=3, **cfg)
    a2.validset = None
    for q in a2.opt_joint.params:               # everything must come from the file
        q.data.add_(0.01)
    a2.load_checkpoint(path)
    a2.fit(4)
    assert a2.epoch == full.epoch == 4 and a2.global_step == full.global_step == 8
    got = _final_state(a2) + [v.detach().clone() for bm in a2.body for v in bm.state_dict().values()]
    names = ["parameters", "joint exp_avg", "joint exp_avg_sq", "joint steps", "pose exp_avg", "pose exp_avg_sq", "pose steps"]
    names += [f"body table {i}" for i in range(len(got) - len(names))]
    for name, x, y in zip(names, got, want):
        assert torch.equal(x, y), (name, int((x != y).sum()), float((x.double() - y.double()).abs().max()))
