"""multiply_amd/trainer.py without a device: the schedule functions against the reference's conditions written out, the learning
rate against torch's MultiStepLR, the float64 Adam yardstick against torch's CPU optimiser, the checkpoint dict, the record table of
mp_adam_multi, and the import."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multiply_amd import trainer as T
from tests import tolerances_trainer as TOL
from tests import trainer_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCHS = [0, 49, 199, 200, 201, 209, 210, 499, 500, 999, 1000]


# ------------------------------------------------------------------------------------------------ schedule
def test_step_plan_over_the_grid():
    n = 0
    for epoch, sam, certain, depth_end, using in itertools.product(EPOCHS, (False, True), (False, True), (False, True), (False, True)):
        cfg = dict(depth_end=depth_end, using_SAM=using, pose_correction_epoch=500)
        got = T.step_plan(epoch, cfg, sam, certain)
        want = R.reference_step_conditions(epoch, sam, certain, depth_end, using)
        # with using_SAM false the reference has no optimiser (cur_opt None, then a crash): that case is the joint optimiser here
        assert got["optimizer"] == (want["cur_opt"] or "joint"), (epoch, sam, certain, depth_end, using)
        assert got["freeze_shape"] == want["freeze"] and got["use_edge_samples"] == want["edge"] and got["mesh_losses"] == want["mesh"]
        n += 1
    assert n == 11 * 16
    # every branch occurs in the grid
    plans = [T.step_plan(e, dict(using_SAM=True, pose_correction_epoch=500), True, c) for e in EPOCHS for c in (False, True)]
    assert {p["optimizer"] for p in plans} == {"joint", "pose"} and any(p["freeze_shape"] for p in plans)
    assert T.step_plan(300, dict(all_edge=True), False, True)["use_edge_samples"]
    assert T.step_plan(205, dict(using_SAM=True, pose_opt_epoch=6), True, True)["optimizer"] == "pose"
    assert T.step_plan(206, dict(using_SAM=True, pose_opt_epoch=6), True, True)["optimizer"] == "joint"


def test_lr_at_is_multistep_lr():
    for lr0, milestones, gamma in ((5e-4, [200, 500], 0.5), (5e-5, [200, 500], 0.5), (1e-3, [3, 3, 7], 0.1)):
        opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr0)
        sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=milestones, gamma=gamma)
        for epoch in range(601):
            assert T.lr_at(epoch, lr0, milestones, gamma) == opt.param_groups[0]["lr"], (epoch, lr0)
            opt.step()
            sch.step()                              # once at every epoch's end (multiply_model.py:219-222)


def test_epoch_end_plan_at_the_period_boundaries():
    cfg = {}
    assert T.epoch_end_plan(0, cfg) == dict(refresh_meshes=False, refresh_masks=True, opt_depth=False)
    for e in (19, 21, 49, 51):
        assert T.epoch_end_plan(e, cfg) == dict(refresh_meshes=False, refresh_masks=False, opt_depth=False)
    assert T.epoch_end_plan(20, cfg)["refresh_meshes"] and not T.epoch_end_plan(20, cfg)["refresh_masks"]
    assert T.epoch_end_plan(50, cfg)["refresh_masks"] and not T.epoch_end_plan(50, cfg)["refresh_meshes"]
    assert T.epoch_end_plan(100, cfg) == dict(refresh_meshes=True, refresh_masks=True, opt_depth=False)
    one = dict(mesh_refresh_period=1, mask_refresh_period=1, depth_end=True, depth_epoch=[1])
    assert T.epoch_end_plan(0, one) == dict(refresh_meshes=False, refresh_masks=True, opt_depth=False)
    assert T.epoch_end_plan(1, one) == dict(refresh_meshes=True, refresh_masks=True, opt_depth=True)
    assert not T.epoch_end_plan(200, dict(depth_epoch=[200]))["opt_depth"]              # depth_end false
    assert T.epoch_end_plan(200, dict(depth_end=True, depth_epoch=[200, 1000]))["opt_depth"]
    assert (T.SCHEDULE_DEFAULTS["mesh_refresh_period"], T.SCHEDULE_DEFAULTS["mask_refresh_period"],
            T.SCHEDULE_DEFAULTS["validation_period"], T.SCHEDULE_DEFAULTS["checkpoint_period"]) == (20, 50, 50, 100)


# ------------------------------------------------------------------------------------------------ the float64 yardstick
def test_float64_adam_against_torch_cpu():
    ps, ms, vs, steps = R.make_state(0)
    gs = R.make_grads(1)
    want = R.table_step64(ps, gs, ms, vs, steps)
    got = R.table_step_torch32(ps, gs, ms, vs, steps)
    assert got[3] == want[3] == [t + (i != R.INACTIVE) for i, t in enumerate(steps)]
    assert np.array_equal(got[0][R.INACTIVE], ps[R.INACTIVE]) and np.array_equal(got[1][R.INACTIVE], ms[R.INACTIVE])
    c_p, c_mv = R.c_of_step(got[0], got[1], got[2], ps, want[0], want[1], want[2])
    print(f"[trainer] torch CPU fp32 Adam against the float64 step: c_p {c_p:.4f}, c_mv {c_mv:.4f}")
    # fp32 arithmetic of a few operations: a handful of ulps, and what tolerances_trainer.py records
    assert 0 < c_p <= TOL.TORCH_CPU_C_P and 0 < c_mv <= TOL.TORCH_CPU_C_MV
    assert TOL.C_P == 2 * TOL.TORCH_CPU_C_P and TOL.C_MV == 2 * TOL.TORCH_CPU_C_MV
    # in float64 torch itself agrees with the yardstick to float64 rounding
    i = 7
    q = torch.tensor(ps[i], dtype=torch.float64)
    opt = torch.optim.Adam([q], lr=R.lr32(R.LRS[1]), betas=(R.BETA1, R.BETA2), eps=R.EPS, foreach=False)
    for k in range(3):
        q.grad = torch.tensor(gs[i], dtype=torch.float64) * (k + 1)
        opt.step()
    p, m, v = np.asarray(ps[i], np.float64), np.zeros(R.SIZES[i]), np.zeros(R.SIZES[i])
    for k in range(3):
        p, m, v = R.adam_step64(p, np.asarray(gs[i], np.float64) * (k + 1), m, v, k, R.lr32(R.LRS[1]))
    # (three steps of a dozen float64 operations each: within 16 float64 ulps of the largest value)
    assert np.abs(q.numpy() - p).max() <= 16 * np.spacing(np.abs(p).max())
    assert np.abs(opt.state[q]["exp_avg"].numpy() - m).max() <= 16 * np.spacing(np.abs(m).max())


# ------------------------------------------------------------------------------------------------ checkpoints
def _cpu_states():
    g = torch.Generator().manual_seed(0)
    model = {"density.beta": torch.rand(1, generator=g), "bg_implicit_network.lin0.weight": torch.rand(4, 3, generator=g)}
    body = [{name + ".weight": torch.rand(3, d, generator=g) for name, d in (("betas", 10), ("global_orient", 3), ("transl", 3),
                                                                             ("body_pose", 69))} for _ in range(2)]
    return model, body


def test_checkpoint_dict_layout_and_round_trip(tmp_path):
    model, body = _cpu_states()
    params = [torch.zeros(4, 3), torch.zeros(1)]
    body_params = [torch.zeros(3, 10), torch.zeros(3, 69)]
    joint = torch.optim.Adam([{"params": params, "lr": 5e-4}, {"params": body_params, "lr": 5e-5}], lr=5e-4, eps=1e-8)
    for p in params + body_params:
        p.grad = torch.ones_like(p)
    joint.step()
    pose = torch.optim.Adam([{"params": body_params, "lr": 5e-5}], lr=5e-4, eps=1e-8)
    scheds = [T.scheduler_state(4, [5e-4, 5e-5], [200, 500], 0.5), T.scheduler_state(4, [5e-5], [200, 500], 0.5)]
    ck = T.checkpoint_dict(4, 15, model, body, [joint.state_dict(), pose.state_dict()], scheds)
    assert set(ck) == {"epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers"}
    assert (ck["epoch"], ck["global_step"]) == (4, 15) and len(ck["optimizer_states"]) == 2 and len(ck["lr_schedulers"]) == 2
    keys = list(ck["state_dict"])
    assert all(k.startswith("model.") or k.startswith("body_model_list.") for k in keys)
    assert "model.density.beta" in keys and "body_model_list.1.body_pose.weight" in keys and "body_model_list.0.betas.weight" in keys
    # the model keys the reference's checkpoint carries (tests/golden/reference_state_keys.npz) get the same prefix
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_state_keys.npz"), allow_pickle=True)
    full = T.checkpoint_dict(0, 0, {str(k): torch.zeros(1) for k in ref["keys"]}, [], [], [])
    assert sorted(full["state_dict"]) == sorted("model." + str(k) for k in ref["keys"])
    path = str(tmp_path / "checkpoints" / T.checkpoint_name(4, 0.25))
    assert os.path.basename(path) == "epoch=0004-loss=0.25.ckpt"
    os.makedirs(os.path.dirname(path))
    torch.save(ck, path)
    assert T.newest_checkpoint(str(tmp_path / "checkpoints")) == path
    back = torch.load(path, weights_only=False)
    m2, b2 = T.split_checkpoint(back)
    assert set(m2) == set(model) and all(torch.equal(m2[k], model[k]) for k in model)
    assert len(b2) == 2 and all(torch.equal(b2[i][k], body[i][k]) for i in range(2) for k in body[i])
    assert back["lr_schedulers"][0]["last_epoch"] == 5 and back["lr_schedulers"][0]["_last_lr"] == [5e-4, 5e-5]
    assert T.scheduler_state(199, [5e-4], [200, 500], 0.5)["_last_lr"] == [2.5e-4]
    # optimizer_states[0] loads into a torch.optim.Adam built over the same shapes
    fresh = [torch.zeros(4, 3), torch.zeros(1)]
    fresh_body = [torch.zeros(3, 10), torch.zeros(3, 69)]
    other = torch.optim.Adam([{"params": fresh, "lr": 1.0}, {"params": fresh_body, "lr": 1.0}], lr=1.0)
    other.load_state_dict(back["optimizer_states"][0])
    assert other.param_groups[0]["lr"] == 5e-4 and other.param_groups[1]["lr"] == 5e-5
    assert float(other.state[fresh[0]]["step"]) == 1 and torch.equal(other.state[fresh_body[1]]["exp_avg"], joint.state[body_params[1]]["exp_avg"])
    # a dict with only a state_dict is accepted; a foreign key is refused
    assert T.split_checkpoint({"state_dict": ck["state_dict"]})[0].keys() == model.keys()
    with pytest.raises(KeyError):
        T.split_checkpoint({"state_dict": {"optimizer.x": torch.zeros(1)}})


def test_device_adam_param_groups_carry_torchs_keys():
    want = set(torch.optim.Adam([torch.zeros(1)], lr=1e-3).param_groups[0]) - {"params"}
    got = T._torch_adam_group_keys(5e-4, (0.9, 0.999), 1e-8)
    assert set(got) == want and got["lr"] == 5e-4 and got["eps"] == 1e-8 and tuple(got["betas"]) == (0.9, 0.999)
    assert got["weight_decay"] == 0 and got["amsgrad"] is False


# ------------------------------------------------------------------------------------------------ the record table
def _addresses(phases, base):
    offs, total = R.layout(phases)
    return [base + 4 * o for o in offs], total


def test_adam_table_blocks_and_access_modes():
    P, _ = _addresses(R.P_PHASE, 0x10000000)
    G, _ = _addresses(R.G_PHASE, 0x20000000)
    M, _ = _addresses(R.M_PHASE, 0x30000000)
    V, _ = _addresses(R.M_PHASE, 0x40000000)
    ns = [int(np.prod(s)) for s in R.SIZES]
    recs = [(P[i], 0 if i == R.INACTIVE else G[i], M[i], V[i], 0x50000000 + 4 * i, ns[i], R.GROUPS[i]) for i in range(len(ns))]
    arr, total = T.adam_table(recs)
    assert C.sizeof(T.MpAdamDesc) == 64 and len(arr) == len(ns)
    # block ranges: ascending from 0, contiguous, and every element of a tensor is covered exactly once by its blocks' strides
    b = 0
    for i, r in enumerate(arr):
        assert r.block0 == b and 1 <= r.n_block <= T.ADAM_MAX_BLOCKS and r.n == ns[i] and r.group == R.GROUPS[i]
        assert r.n_block == min(-(-ns[i] // T.ADAM_BLOCK_ELEMS), T.ADAM_MAX_BLOCKS)
        b += r.n_block
        seen = np.zeros(ns[i], dtype=np.int64)
        for blk in range(r.n_block):              # the kernel's scalar-path indexing: i = blk*256 + tid, stride n_block*256
            for start in range(blk * 256, ns[i], r.n_block * 256):
                seen[start:start + 256] += 1
        assert (seen == 1).all()
    assert total == b and arr[-1].n_block == T.ADAM_MAX_BLOCKS and ns[-1] > T.ADAM_MAX_BLOCKS * T.ADAM_BLOCK_ELEMS
    # modes: the inactive record has no gradient yet (judged on p, m, v alone); the others as trainer_reference.MODES says
    assert [r.mode for r in arr] == R.MODES and arr[R.INACTIVE].g is None
    assert arr[6].mode == T.ADAM_SCALAR                                    # moments elsewhere within 16 bytes: scalar path
    T.set_gradient(arr[0], G[0] + 4)
    assert arr[0].mode == T.ADAM_VEC_G4 and arr[0].g == G[0] + 4            # the gradient alone off: dword reads of it
    T.set_gradient(arr[0], 0)
    assert arr[0].g is None
    assert T.access_mode(0x1002, 0x2002, 0x3002, 0x4002) == T.ADAM_SCALAR   # not even 4-byte aligned
    # a smaller cap strides more
    arr2, total2 = T.adam_table(recs, max_blocks=2)
    assert [r.n_block for r in arr2] == [1, 1, 1, 1, 1, 1, 1, 2] and total2 == 9
    # the header declares the same record and the same constants
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    assert "MP_ADAM_SCALAR = 0, MP_ADAM_VEC = 1, MP_ADAM_VEC_G4 = 2" in hdr
    assert "int group, block0, n_block, mode;" in hdr
    from multiply_amd import hip
    rt, at = hip.header_prototypes()["mp_adam_multi"]
    assert rt is C.c_int and at == [hip.DevPtr, C.c_int, C.c_int, hip.DevPtr, hip.DevPtr, C.c_double, C.c_double, C.c_double, hip.DevPtr]
    assert "mp_adam_multi" not in hip.VALUE_RETURNING


# ------------------------------------------------------------------------------------------------ import
def test_trainer_imports_without_a_device():
    code = ("import sys; import multiply_amd.trainer as T; from multiply_amd import hip; "
            "assert hip._lib is None, 'the library was loaded at import'; print(T.lr_at(200, 1.0, [200], 0.5))")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO)
    assert r.returncode == 0 and r.stdout.strip() == "0.5", r.stderr[-2000:]
