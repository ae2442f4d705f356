"""The trainer on the device: mp_adam_multi against the float64 step of tests/trainer_reference.py (bounds:
tests/tolerances_trainer.py), DeviceAdam's state against torch.optim.Adam's, and Trainer's step / fit / resume / test on a small
written sequence."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import tolerances_trainer as TOL
from tests import trainer_reference as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


# ================================================================================================ the kernel (tests 1 - 3)
class RawTable:
    """the table of trainer_reference on the device, every tensor a view into one flat buffer per role at the offsets the reference
    lists; launched through the C entry point as it is"""

    def __init__(self, ps, ms, vs, steps, max_blocks=None):
        from multiply_amd import trainer as T
        self.T = T
        self.ns = [int(np.prod(s)) for s in R.SIZES]
        (self.op, tp), (self.og, tg), (self.om, tm) = R.layout(R.P_PHASE), R.layout(R.G_PHASE), R.layout(R.M_PHASE)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.P, self.G = torch.full((tp,), 7.0, **f32), torch.full((tg,), 7.0, **f32)       # (7: the gaps between tensors)
        self.M, self.V = torch.full((tm,), 7.0, **f32), torch.full((tm,), 7.0, **f32)
        self.steps = torch.tensor([float(t) for t in steps], **f32)
        for i, n in enumerate(self.ns):
            self.view(self.P, self.op, i).copy_(torch.from_numpy(np.asarray(ps[i], np.float32).reshape(-1)))
            self.view(self.M, self.om, i).copy_(torch.from_numpy(np.asarray(ms[i], np.float32).reshape(-1)))
            self.view(self.V, self.om, i).copy_(torch.from_numpy(np.asarray(vs[i], np.float32).reshape(-1)))
        self.lr = torch.tensor(R.LRS, **f32)
        self.max_blocks = T.ADAM_MAX_BLOCKS if max_blocks is None else max_blocks
        self.gaps = [self._gap(b, o) for b, o in ((self.P, self.op), (self.M, self.om), (self.V, self.om))]

    def view(self, buf, offs, i):
        return buf[offs[i]:offs[i] + self.ns[i]]

    def _gap(self, buf, offs):
        keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
        for i in range(len(self.ns)):
            keep[offs[i]:offs[i] + self.ns[i]] = False
        return keep

    def launch(self, gs, skip=None):
        from multiply_amd import hip
        recs = []
        for i in range(len(self.ns)):
            g = 0
            if gs[i] is not None:
                self.view(self.G, self.og, i).copy_(torch.from_numpy(np.asarray(gs[i], np.float32).reshape(-1)))
                g = self.view(self.G, self.og, i).data_ptr()
            recs.append((self.view(self.P, self.op, i).data_ptr(), g, self.view(self.M, self.om, i).data_ptr(),
                         self.view(self.V, self.om, i).data_ptr(), self.steps.data_ptr() + 4 * i, self.ns[i], R.GROUPS[i]))
        arr, total = self.T.adam_table(recs, self.max_blocks)
        self.modes = [r.mode for r in arr]
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        hip.lib().mp_adam_multi(tab, len(recs), total, self.lr, skip, R.BETA1, R.BETA2, R.EPS, hip.stream())
        torch.cuda.synchronize()

    def state(self):
        get = lambda buf, offs: [self.view(buf, offs, i).cpu().numpy().reshape(R.SIZES[i]) for i in range(len(self.ns))]
        return get(self.P, self.op), get(self.M, self.om), get(self.V, self.om), self.steps.cpu().tolist()

    def gaps_untouched(self):
        return all(bool((buf[keep] == 7.0).all()) for buf, keep in zip((self.P, self.M, self.V), self.gaps))


def _check_step(got, before, want, what):
    """test 1's bound per element, on every tensor that stepped; bit-identity (count included) on those that did not"""
    gp, gm, gv, gt = got
    ps, ms, vs, ts = before
    wp, wm, wv, wt = want
    worst = {"p": 0.0, "mv": 0.0}
    for i in range(len(ps)):
        if wp[i] is ps[i]:                                                     # no gradient: nothing may change
            assert np.array_equal(gp[i], ps[i]) and np.array_equal(gm[i], ms[i]) and np.array_equal(gv[i], vs[i]), (what, i)
            assert gt[i] == ts[i], (what, i)
            continue
        assert gt[i] == wt[i], (what, i, gt[i], wt[i])
        dp = np.abs(wp[i] - np.asarray(ps[i], np.float64))
        err = np.abs(gp[i].astype(np.float64) - wp[i])
        bound = R.half_ulp32(wp[i]) + TOL.C_P * 2.0 ** -24 * dp
        worst["p"] = max(worst["p"], float(((err - R.half_ulp32(wp[i])) / np.maximum(2.0 ** -24 * dp, 1e-300)).max()))
        assert (err <= bound).all(), (what, i, float((err - bound).max()))
        for g_, w_ in ((gm[i], wm[i]), (gv[i], wv[i])):
            e = np.abs(g_.astype(np.float64) - w_)
            nz = np.abs(w_) >= TOL.FLT_MIN
            if nz.any():
                worst["mv"] = max(worst["mv"], float((e[nz] / np.abs(w_[nz])).max() / 2.0 ** -24))
            bad = e > TOL.C_MV * (2.0 ** -24 * np.abs(w_) + TOL.SUBNORMAL_SPACING)
            assert not bad.any(), (what, i, "want", w_[bad][:4], "error", e[bad][:4])
    print(f"[trainer] {what}: needs c_p {worst['p']:.3f} (bound {TOL.C_P}), c_mv {worst['mv']:.3f} (bound {TOL.C_MV})")


def test_adam_kernel_one_step_against_float64():
    ps, ms, vs, steps = R.make_state(0)
    gs = R.make_grads(1)
    assert gs[R.INACTIVE] is None and not gs[R.ZERO_GRAD].any() and ms[R.ZERO_GRAD].any() and 0 < R.INACTIVE < len(gs) - 1
    assert set(steps) == {0, 999} and sorted(set(R.G_PHASE)) == [0, 1, 2, 3]
    tab = RawTable(ps, ms, vs, steps)
    tab.launch(gs)
    assert tab.modes == R.MODES and set(tab.modes) == {0, 1, 2}                # all three access paths ran
    _check_step(tab.state(), (ps, ms, vs, steps), R.table_step64(ps, gs, ms, vs, steps), "one step")
    assert tab.gaps_untouched()
    # the zero gradient still moves the parameter by its momentum
    assert not np.array_equal(tab.state()[0][R.ZERO_GRAD], ps[R.ZERO_GRAD])
    # a smaller cap on the blocks per tensor (more strides) gives the same bits
    tab2 = RawTable(ps, ms, vs, steps, max_blocks=3)
    tab2.launch(gs)
    for a, b in zip(tab.state()[:3], tab2.state()[:3]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # argument errors, empty table
    from multiply_amd import hip
    L, st = hip.lib(), hip.stream()
    L.mp_adam_multi(None, 0, 0, None, None, 0.9, 0.999, 1e-8, st)
    with pytest.raises(RuntimeError, match=r"^mp_adam_multi failed with code -1$"):
        L.mp_adam_multi(None, 2, 2, tab.lr, None, 0.9, 0.999, 1e-8, st)
    with pytest.raises(RuntimeError, match=r"^mp_adam_multi failed with code -2$"):
        L.mp_adam_multi(tab.lr, 1, 1, tab.lr, None, 1.0, 0.999, 1e-8, st)


def test_adam_kernel_twenty_chained_steps():
    ps, ms, vs, steps = R.make_state(0)
    grads = []
    for s in range(TOL.CHAIN_STEPS):
        gs = R.make_grads(100 + s)
        grads.append(gs)
    tab = RawTable(ps, ms, vs, steps)
    p64, m64, v64, t64 = ps, ms, vs, steps
    for gs in grads:
        tab.launch(gs)
        p64, m64, v64, t64 = R.table_step64(p64, gs, m64, v64, t64)
    t32 = R.table_step_torch32(ps, grads[0], ms, vs, steps, n_steps=TOL.CHAIN_STEPS, grads_per_step=grads)
    gp, gm, gv, gt = tab.state()
    assert gt == t64
    for i in range(len(ps)):
        if i == R.INACTIVE:
            assert np.array_equal(gp[i], ps[i]) and gt[i] == steps[i]
            continue
        dev_kernel = float(np.abs(gp[i].astype(np.float64) - p64[i]).max())
        dev_torch = float(np.abs(t32[0][i].astype(np.float64) - p64[i]).max())
        floor = TOL.CHAIN_STEPS * float(R.half_ulp32(np.abs(p64[i]).max()))
        print(f"[trainer] 20 steps, tensor {i} {R.SIZES[i]}: max |p - p64| kernel {dev_kernel:.3e}, torch CPU fp32 {dev_torch:.3e}, "
              f"20 x half ulp {floor:.3e}")
        assert dev_kernel <= max(2 * dev_torch, floor), i


def test_adam_kernel_skip_flag():
    ps, ms, vs, steps = R.make_state(0)
    gs = R.make_grads(1)
    tab = RawTable(ps, ms, vs, steps)
    flag = torch.ones(1, dtype=torch.uint8, device=DEV)
    tab.launch(gs, skip=flag)
    gp, gm, gv, gt = tab.state()
    for i in range(len(ps)):
        assert np.array_equal(gp[i], ps[i]) and np.array_equal(gm[i], ms[i]) and np.array_equal(gv[i], vs[i]), i
    assert gt == [float(t) for t in steps]
    flag.zero_()
    tab.launch(gs, skip=flag)
    first = RawTable(ps, ms, vs, steps)
    first.launch(gs)
    for a, b in zip(tab.state(), first.state()):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert tab.state()[3] == [t + (i != R.INACTIVE) for i, t in enumerate(steps)]


# ================================================================================================ DeviceAdam (tests 4, 5)
def _device_adam(ps):
    from multiply_amd.trainer import DeviceAdam
    params = [torch.tensor(np.asarray(p, np.float32), device=DEV) for p in ps]
    groups = [{"params": [q for q, g in zip(params, R.GROUPS) if g == k], "lr": lr} for k, lr in enumerate(R.LRS)]
    order = [i for k in range(len(R.LRS)) for i, g in enumerate(R.GROUPS) if g == k]
    return DeviceAdam(groups, betas=(R.BETA1, R.BETA2), eps=R.EPS), params, order


def _set_grads(params, gs, flat=None):
    for q, g in zip(params, gs):
        q.grad = None if g is None else torch.tensor(np.asarray(g, np.float32), device=DEV)


def test_state_interop_with_torch_adam():
    ps, _, _, _ = R.make_state(0)
    fresh = [np.zeros(s, np.float32) for s in R.SIZES]
    opt, params, order = _device_adam(ps)
    grads = [R.make_grads(1)] * 4                   # every step on the same gradients (test 1's)
    for s in range(3):
        _set_grads(params, grads[s])
        opt.step()
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and [g["params"] for g in sd["param_groups"]] == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert order.index(R.INACTIVE) not in sd["state"] and len(sd["state"]) == 7       # never stepped: no state, as in torch
    st0 = sd["state"][0]
    assert set(st0) == {"step", "exp_avg", "exp_avg_sq"} and st0["step"].dtype == torch.float32 and float(st0["step"]) == 3
    # -> torch.optim.Adam on CPU copies, one more step on both sides
    cpu_sd = {"state": {k: {n: t.cpu() for n, t in v.items()} for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
    before = [q.detach().cpu().numpy().copy() for q in params]
    mom = [tuple(t.cpu().numpy().copy() for t in opt.moments(order.index(i))) for i in range(len(ps))]
    topt, tparams, torder = R.torch_cpu_optimizer(before)
    assert torder == order
    topt.load_state_dict(cpu_sd)
    for q, g in zip(tparams, grads[3]):
        q.grad = None if g is None else torch.tensor(g)
    topt.step()
    _set_grads(params, grads[3])
    opt.step()
    torch.cuda.synchronize()
    ms, vs = [m for m, _ in mom], [v for _, v in mom]
    steps = [0 if i == R.INACTIVE else 3 for i in range(len(ps))]
    want = R.table_step64(before, grads[3], ms, vs, steps)
    got_dev = ([q.detach().cpu().numpy() for q in params], [opt.moments(order.index(i))[0].cpu().numpy() for i in range(len(ps))],
               [opt.moments(order.index(i))[1].cpu().numpy() for i in range(len(ps))], [float(opt.steps[order.index(i)]) for i in range(len(ps))])
    _check_step(got_dev, (before, ms, vs, steps), want, "DeviceAdam step 4")
    tstate = topt.state_dict()["state"]
    got_torch = ([q.detach().numpy() for q in tparams],
                 [tstate[order.index(i)]["exp_avg"].numpy() if order.index(i) in tstate else ms[i] for i in range(len(ps))],
                 [tstate[order.index(i)]["exp_avg_sq"].numpy() if order.index(i) in tstate else vs[i] for i in range(len(ps))],
                 [float(tstate[order.index(i)]["step"]) if order.index(i) in tstate else 0.0 for i in range(len(ps))])
    _check_step(got_torch, (before, ms, vs, steps), want, "torch CPU step 4 from DeviceAdam's state")
    # the reverse direction: torch's state after that step -> a fresh DeviceAdam; one more step against float64
    now = [q.detach().numpy().copy() for q in tparams]
    opt2, params2, _ = _device_adam(now)
    opt2.load_state_dict(topt.state_dict())
    assert opt2.param_groups[1]["lr"] == R.LRS[1]
    ms2, vs2, steps2 = got_torch[1], got_torch[2], [int(t) for t in got_torch[3]]
    _set_grads(params2, grads[0])
    opt2.step()
    torch.cuda.synchronize()
    want2 = R.table_step64(now, grads[0], ms2, vs2, steps2)
    got2 = ([q.detach().cpu().numpy() for q in params2], [opt2.moments(order.index(i))[0].cpu().numpy() for i in range(len(ps))],
            [opt2.moments(order.index(i))[1].cpu().numpy() for i in range(len(ps))], [float(opt2.steps[order.index(i)]) for i in range(len(ps))])
    _check_step(got2, (now, ms2, vs2, steps2), want2, "DeviceAdam step from torch's state")
    del fresh


def test_device_adam_step_makes_no_host_synchronisation():
    ps, _, _, _ = R.make_state(0)
    opt, params, order = _device_adam(ps)
    gs = R.make_grads(1)
    _set_grads(params, gs)
    opt.step()                                         # builds the table
    loss = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    before = [q.detach().clone() for q in params]
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step(skip=torch.isnan(loss))
        opt.set_lr(0, 1e-4)
        opt.step(skip=torch.isnan(loss / 0))           # NaN: skipped
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(q.grad is None for q in params) and opt.param_groups[0]["lr"] == 1e-4
    assert opt.steps.cpu().tolist() == [0.0 if i == order.index(R.INACTIVE) else 2.0 for i in range(8)]
    assert not torch.equal(params[0], before[0])


# ================================================================================================ Trainer (tests 6 - 9)
def _build(tmp, name="run", seq=None, predictor=None, seed=3, **cfg):
    """a Trainer over a written 3-frame 64 x 64 sequence with 2 persons, 96 rays per step"""
    import warnings
    warnings.filterwarnings("ignore")
    from multiply_amd import trainer as T
    from multiply_amd.config import load_config
    from multiply_amd.synthetic import make_smpl_tables, write_sequence
    root = os.path.join(str(tmp), "seq") if seq is None else seq
    if not os.path.exists(root):
        write_sequence(root, n_frames=3, H=64, W=64, num_person=2)
    opt = load_config()
    for k, v in dict(valid_res_up=1, test_res_up=1, mesh_res_up=1, mask_res_up=1, pose_correction_epoch=500, **cfg).items():
        opt[k] = v
    tr = T.build_trainer(root, os.path.join(str(tmp), name), opt=opt, dataset_opt=dict(num_sample=96, pixel_per_batch=2048),
                         sam_predictor=predictor, smpl_tables=make_smpl_tables(0), seed=seed, log=lambda *a: None)
    return tr


def _snapshot(tr):
    snap = {}
    for name, opt in tr.optimizers.items():
        snap[name] = dict(p=[q.detach().clone() for q in opt.params], m=opt.exp_avg.clone(), v=opt.exp_avg_sq.clone(),
                          t=opt.steps.clone())
    return snap


def _unchanged(tr, snap, name, only=None, state_only=False):
    """state_only: the moments and counts alone (the two optimisers share the body tables: a joint step moves the pose
    optimiser's parameters, never its state)"""
    opt, s = tr.optimizers[name], snap[name]
    for i, q in enumerate(opt.params):
        if only is not None and i not in only:
            continue
        m, v = opt.moments(i)
        o, n = opt.offsets[i], q.numel()
        assert (state_only or torch.equal(q.detach(), s["p"][i])) and torch.equal(m.reshape(-1), s["m"][o:o + n]), (name, i)
        assert torch.equal(v.reshape(-1), s["v"][o:o + n]) and float(opt.steps[i]) == float(s["t"][i]), (name, i)


def _against_torch_cpu(tr, snap, name, what):
    """every tensor of optimiser `name` with a gradient: one torch.optim.Adam step in float64 on CPU copies of the pre-step state with
    the step's own .grad (torch's arithmetic, no fp32 rounding: the float64 yardstick) -> test 1's bound; without: bit-identical"""
    opt, s = tr.optimizers[name], snap[name]
    active = [i for i, q in enumerate(opt.params) if q.grad is not None]
    _unchanged(tr, snap, name, only=set(range(len(opt.params))) - set(active))
    before, ms, vs, ts, gs, got, lrs = [], [], [], [], [], ([], [], [], []), []
    for i in active:
        q, (m, v) = opt.params[i], opt.moments(i)
        o, n = opt.offsets[i], q.numel()
        before.append(s["p"][i].cpu().numpy()); ms.append(s["m"][o:o + n].reshape(q.shape).cpu().numpy())
        vs.append(s["v"][o:o + n].reshape(q.shape).cpu().numpy()); ts.append(float(s["t"][i])); gs.append(q.grad.cpu().numpy())
        lrs.append(R.lr32(opt.param_groups[opt.group_of[i]]["lr"]))
        for dst, val in zip(got, (q.detach().cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), float(opt.steps[i]))):
            dst.append(val)
    want = ([], [], [], [])
    for p0, m0, v0, t0, g, lr in zip(before, ms, vs, ts, gs, lrs):
        q = torch.tensor(p0, dtype=torch.float64)
        o = torch.optim.Adam([q], lr=lr, betas=(R.BETA1, R.BETA2), eps=R.EPS, foreach=False)
        if t0:
            o.load_state_dict({"state": {0: {"step": torch.tensor(t0), "exp_avg": torch.tensor(m0, dtype=torch.float64),
                                             "exp_avg_sq": torch.tensor(v0, dtype=torch.float64)}},
                               "param_groups": o.state_dict()["param_groups"]})
        q.grad = torch.tensor(g, dtype=torch.float64)
        o.step()
        st = o.state[q]
        for dst, val in zip(want, (q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), float(st["step"]))):
            dst.append(val)
    assert active and all(np.isfinite(g).all() for g in gs)
    _check_step(got, (before, ms, vs, ts), want, what)
    return active


@pytest.fixture(scope="module")
def step_trainer(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("steps"), using_SAM=True)


def _fresh_optimizers(tr):
    """new optimiser states over the same parameters (each plan is checked from a first step)"""
    from multiply_amd.trainer import DeviceAdam
    for name in ("joint", "pose"):
        old = tr.optimizers[name]
        new = DeviceAdam([{"params": g["params"], "lr": g["lr"]} for g in old.param_groups], eps=1e-8)
        tr.optimizers[name] = new
    tr.opt_joint, tr.opt_pose = tr.optimizers["joint"], tr.optimizers["pose"]


def _item(tr, frame, sam=False, certain=True, nan=False):
    inputs, targets = tr.trainset[frame]
    inputs["is_certain"] = certain
    if sam:
        H, W = tr.trainset.img_size
        rs = np.random.RandomState(7)
        inputs["org_sam_mask"] = torch.tensor(rs.normal(0, 4.0, (H, W, 2)), dtype=torch.float32, device=DEV)
        inputs["sam_mask"] = torch.tensor(rs.normal(0, 4.0, (inputs["uv"].shape[0], 2)), dtype=torch.float32, device=DEV)
    if nan:
        targets["rgb"] = targets["rgb"] * float("nan")
    return inputs, targets


def test_training_step_of_every_plan(step_trainer):
    tr = step_trainer
    nets = tr.frozen_ids
    n_body = len(tr.opt_pose.params)
    # ---- joint step
    _fresh_optimizers(tr)
    snap = _snapshot(tr)
    plan, lo = tr.training_step(_item(tr, 1), 301)
    torch.cuda.synchronize()
    assert plan == dict(optimizer="joint", freeze_shape=False, use_edge_samples=False, mesh_losses=False) and torch.isfinite(lo["loss"]).all()
    active = _against_torch_cpu(tr, snap, "joint", "joint step")
    _unchanged(tr, snap, "pose", state_only=True)                             # the other optimiser's state: untouched
    stepped = {id(tr.opt_joint.params[i]) for i in active}
    assert stepped & nets and len(stepped - nets) > n_body // 2                # networks and body tables both moved
    assert tr.global_step == 1
    # ---- frozen-shape step: an uncertain frame before pose_correction_epoch
    _fresh_optimizers(tr)
    snap = _snapshot(tr)
    plan, _ = tr.training_step(_item(tr, 2, certain=False), 301)
    torch.cuda.synchronize()
    assert plan["optimizer"] == "joint" and plan["freeze_shape"] and plan["use_edge_samples"] and not plan["mesh_losses"]
    active = _against_torch_cpu(tr, snap, "joint", "frozen-shape step")
    assert not ({id(tr.opt_joint.params[i]) for i in active} & nets)           # the four network lists: excluded, bit-identical
    assert all(p.requires_grad for p in tr.opt_joint.params)                   # ... and unfrozen again afterwards
    _unchanged(tr, snap, "pose", state_only=True)
    # ---- pose step: SAM labels, epoch 300 (300 % 10 < 1)
    _fresh_optimizers(tr)
    snap = _snapshot(tr)
    plan, lo = tr.training_step(_item(tr, 1, sam=True), 300)
    torch.cuda.synchronize()
    assert plan == dict(optimizer="pose", freeze_shape=False, use_edge_samples=False, mesh_losses=True)
    assert torch.isfinite(lo["loss"]).all() and "depth_order_loss_pyrender" in lo
    _against_torch_cpu(tr, snap, "pose", "pose step")
    snap_joint_only = {"joint": snap["joint"]}
    for i, q in enumerate(tr.opt_joint.params):                                # the joint optimiser's state and every network: untouched
        if id(q) not in {id(b) for b in tr.opt_pose.params}:
            assert torch.equal(q.detach(), snap_joint_only["joint"]["p"][i]), i
    assert float(tr.opt_joint.steps.sum()) == 0 and not tr.opt_joint.exp_avg.any()
    # ---- a NaN target: nothing changes anywhere
    snap = _snapshot(tr)
    plan, lo = tr.training_step(_item(tr, 0, nan=True), 301)
    torch.cuda.synchronize()
    assert torch.isnan(lo["loss"]).all() and plan["optimizer"] == "joint"
    _unchanged(tr, snap, "joint")
    _unchanged(tr, snap, "pose")
    log = tr.epoch_log(301)
    assert log["steps"] == 4 and log["skipped_nan"] == 1 and np.isfinite(log["loss"])


def _load_ply_faces(path):
    from multiply_amd.metrics import load_ply
    m = load_ply(path)
    v, f = (m["vertices"], m["faces"]) if isinstance(m, dict) else (m[0], m[1])
    return np.asarray(v.cpu() if torch.is_tensor(v) else v), np.asarray(f.cpu() if torch.is_tensor(f) else f)


def test_fit_two_epochs_with_every_stage(tmp_path):
    from multiply_amd import trainer as T
    from tests.sam_standin import StandInPredictor
    tr = _build(tmp_path, predictor=StandInPredictor(), using_SAM=True, mesh_refresh_period=1, mask_refresh_period=1,
                validation_period=1, checkpoint_period=1, depth_end=True, depth_epoch=[1], it_per_loop=2, depth_frames=[1],
                sched_milestones=[1], sched_factor=0.5)
    out = tr.out_dir
    meshes0 = [v.clone() for v in tr.model.mesh_v_cano_list]
    body0 = [{k: v.detach().clone() for k, v in bm.state_dict().items()} for bm in tr.body]
    seen_body = {}
    depth = tr.opt_depth

    def spy(epoch):                                                           # the body tables around the depth stage
        seen_body["before"] = [{k: v.detach().clone() for k, v in bm.state_dict().items()} for bm in tr.body]
        r = depth(epoch)
        seen_body["after"] = [{k: v.detach().clone() for k, v in bm.state_dict().items()} for bm in tr.body]
        return r
    tr.opt_depth = spy
    logs = tr.fit(2)
    torch.cuda.synchronize()
    assert [l["epoch"] for l in logs] == [0, 1] and all(l["steps"] == 3 and np.isfinite(l["loss"]) for l in logs) and tr.global_step == 6
    # learning rates: the device scalars follow lr_at (milestone at epoch 1; after fit they hold epoch 2's)
    lr0 = tr.lr0
    assert logs[0]["lr"] == lr0 and logs[1]["lr"] == T.lr_at(1, lr0, [1], 0.5) == 0.5 * lr0
    assert tr.opt_joint.lr.cpu().tolist() == [np.float32(T.lr_at(2, lr0, [1], 0.5)), np.float32(T.lr_at(2, 0.1 * lr0, [1], 0.5))]
    assert tr.opt_pose.lr.cpu().tolist() == [np.float32(T.lr_at(2, 0.1 * lr0, [1], 0.5))]
    # canonical meshes replaced (epoch 1)
    assert all(v.shape != m0.shape or not torch.equal(v, m0) for v, m0 in zip(tr.model.mesh_v_cano_list, meshes0))
    assert all(fv.shape[2:] == (3, 3) for fv in tr.model.mesh_face_vertices_list)
    # stage files, with the shapes their readers expect
    for e in (0, 1):
        m = np.load(os.path.join(out, f"stage_instance_mask/{e:05d}/all_person_smpl_mask.npy"))
        k = np.load(os.path.join(out, f"stage_instance_mask/{e:05d}/2d_keypoint.npy"))
        s = np.load(os.path.join(out, f"stage_sam_mask/{e:05d}/sam_opt_mask.npy"))
        assert m.shape == (3, 2, 64, 64) and m.dtype == bool and k.shape == (3, 2, 27, 2) and s.shape == (3, 2, 64, 64)
        for name in ("rendering", "normal", "fg_rendering"):
            for vid in (-1, 0, 1):
                from PIL import Image
                img = Image.open(os.path.join(out, f"{name}/{e}_person{vid}.png"))
                assert img.size == (64, 128 if name == "rendering" else 64), (name, e, vid, img.size)
        for p in (0, 1):
            v, f = _load_ply_faces(os.path.join(out, f"rendering/{e}_{p}.ply"))
            assert v.shape[1] == 3 and f.shape[1] == 3 and f.max() < v.shape[0]
    cks = sorted(glob.glob(os.path.join(out, "checkpoints", "epoch=*.ckpt")))
    assert [os.path.basename(c)[:10] for c in cks] == ["epoch=0000", "epoch=0001"] and os.path.exists(os.path.join(out, "checkpoints", "last.ckpt"))
    ck = torch.load(cks[-1], map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["global_step"] == 6 and len(ck["optimizer_states"]) == 2
    ref = np.load(os.path.join(REPO, "tests", "golden", "reference_state_keys.npz"), allow_pickle=True)
    model_keys = {k[len("model."):] for k in ck["state_dict"] if k.startswith("model.")}
    assert {str(k) for k in ref["param_keys"]} <= model_keys
    assert "body_model_list.1.transl.weight" in ck["state_dict"]
    # the dataset picked the new masks up (epoch 1's items carried them)
    assert tr.trainset.pre_mask_path.endswith("stage_sam_mask/00000/sam_opt_mask.npy") or tr.trainset.pre_mask_path.endswith("stage_sam_mask/00001/sam_opt_mask.npy")
    assert tr.trainset.pre_mask is not None and tuple(tr.trainset.pre_mask.shape) == (3, 64, 64, 2)
    # opt_depth: one frame, two iterations, only that frame's translation rows moved
    hist = tr.last_depth_history
    assert len(hist) == 1 and len(hist[0]) == 2
    for before, after in zip(seen_body["before"], seen_body["after"]):
        for k in before:
            if k == "transl.weight":
                assert torch.equal(before[k][[0, 2]], after[k][[0, 2]]) and not torch.equal(before[k][1], after[k][1])
            else:
                assert torch.equal(before[k], after[k]), k
    del body0


def _final_state(tr):
    """[all parameters as one vector, then exp_avg, exp_avg_sq and the counts of the joint and of the pose optimiser]"""
    torch.cuda.synchronize()
    out = [torch.cat([q.detach().reshape(-1) for q in tr.opt_joint.params])]
    for o in (tr.opt_joint, tr.opt_pose):
        out += [o.exp_avg.clone(), o.exp_avg_sq.clone(), o.steps.clone()]
    return out


def _difference(x, y):
    """(median, 99th percentile, maximum) of |x - y|"""
    d = (x - y).abs().flatten().sort().values
    n = d.numel()
    return float(d[n // 2]), float(d[min(n - 1, (99 * n) // 100)]), float(d[-1])


def test_resume_equals_an_uninterrupted_run(tmp_path):
    """Run A: fit(1), save, load into a fresh trainer (perturbed first, so that everything must come from the file), fit(2); four
    uninterrupted fit(2) runs of the same seeds beside it.

    What is exact is asserted exactly: the loaded trainer's parameters and both optimiser states are the saved bits; after the
    resumed epoch the step counts, the epoch / step counters and the position of the two host random streams equal an
    uninterrupted run's (same frames, same rays).

    The rest is compared with the run-to-run difference.  The training kernels accumulate gradients with float atomics, so two
    uninterrupted runs differ; measured on this sequence (six steps): exp_avg up to 4e-7, exp_avg_sq up to 1.8e-10, parameters
    below 1e-6 on 97 - 99 % of the elements and 6e-5 ... 2e-4 on a few (Adam's normalised step turns a last-bit difference of a
    near-zero gradient into a step of the size of the learning rate; the maximum takes a handful of discrete values).  Resumed runs
    were measured to lie in the same cloud (seven runs, every pairwise difference: resumed-uninterrupted, resumed-resumed and
    uninterrupted-uninterrupted have the same medians, tails and maxima).  But a difference between two runs is a random draw: a
    correct resumed run exceeds ONE measured pair every other time, and the largest of k pairs about once in k + 1.  So the
    run-to-run difference is taken as the largest of the six pairs of four runs, A is compared with its nearest of the four, and --
    the one widening beyond the issue's wording -- twice that value is allowed.  A restore that loses anything (moments, counts,
    random streams) moves exp_avg by 1e-4 and every parameter by 1e-4 ... 1e-3: hundreds of times the noise.  Where the four runs
    agree to the bit, A must too."""
    import itertools
    seq = os.path.join(str(tmp_path), "seq")
    big = dict(mesh_refresh_period=10 ** 6, mask_refresh_period=10 ** 6, validation_period=10 ** 6, checkpoint_period=10 ** 6)
    refs = []
    for name in ("B", "C", "D", "E"):
        tr = _build(tmp_path, name, seq=seq, **big)
        tr.validset = None
        tr.fit(2)
        refs.append(_final_state(tr))
    a1 = _build(tmp_path, "A", seq=seq, **big)
    a1.validset = None
    a1.fit(1)
    path = a1.save_checkpoint(os.path.join(a1.out_dir, "checkpoints", "epoch=0000-loss=x.ckpt"))
    saved = _final_state(a1)
    a2 = _build(tmp_path, "A", seq=seq, **big)
    a2.validset = None
    for q in a2.opt_joint.params:
        q.data.add_(0.01)
    a2.load_checkpoint(path)
    assert a2.epoch == 1 and a2.global_step == 3
    assert all(torch.equal(x, y) for x, y in zip(_final_state(a2), saved))              # the restore is exact
    for q in a2.opt_joint.params:
        q.data.add_(0.01)
    a2.fit(2, resume=True)                                                               # is_continue: the newest epoch=*.ckpt
    assert a2.epoch == tr.epoch == 2 and a2.global_step == tr.global_step == 6 and path.endswith("epoch=0000-loss=x.ckpt")
    assert a2.rng.rand() == tr.rng.rand() and a2.trainset.rng.rand() == tr.trainset.rng.rand()      # the same draws were made
    got = _final_state(a2)
    names = ["parameters", "joint exp_avg", "joint exp_avg_sq", "joint steps", "pose exp_avg", "pose exp_avg_sq", "pose steps"]
    for k, (name, a) in enumerate(zip(names, got)):
        pairs = [_difference(x[k], y[k]) for x, y in itertools.combinations(refs, 2)]
        mine = [_difference(a, x[k]) for x in refs]
        rr = [max(p[j] for p in pairs) for j in range(3)]
        res = [min(m[j] for m in mine) for j in range(3)]
        print(f"[trainer] resume, {name}: |resumed - nearest uninterrupted| median {res[0]:.2e} p99 {res[1]:.2e} max {res[2]:.2e}; "
              f"uninterrupted pairs up to {rr[0]:.2e} / {rr[1]:.2e} / {rr[2]:.2e}")
        if rr[2] == 0 or "steps" in name:
            assert torch.equal(a, refs[0][k]), name
        else:
            assert all(r <= 2 * w for r, w in zip(res, rr)), (name, res, rr)
    assert float(refs[0][3].max()) == 6 and float(refs[0][6].sum()) == 0      # six joint steps; the pose optimiser never stepped


def test_test_run_on_one_frame(tmp_path):
    from PIL import Image
    tr = _build(tmp_path)
    tr.test(frames=[1])
    out = tr.out_dir
    for folder in ("test_rendering", "test_fg_rendering", "test_normal", "test_mask"):
        for vid in (-1, 0, 1):
            img = Image.open(os.path.join(out, folder, str(vid), "0001.png"))
            assert img.size == (64, 64), (folder, vid)
    for p in (0, 1):
        assert Image.open(os.path.join(out, "test_instance_mask", str(p), "0001.png")).size == (64, 64)
        vc, fc = _load_ply_faces(os.path.join(out, "test_mesh", str(p), "0001_canonical.ply"))
        vd, fd = _load_ply_faces(os.path.join(out, "test_mesh", str(p), "0001_deformed.ply"))
        assert np.array_equal(fc, fd) and vc.shape == vd.shape and not np.array_equal(vc, vd)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_images.py"), os.path.join(out, "test_rendering", "-1"),
                        os.path.join(out, "test_rendering", "-1")], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["n_frames"] == 1 and abs(res["mean_ssim"] - 1.0) < 1e-6          # a rendering against itself
