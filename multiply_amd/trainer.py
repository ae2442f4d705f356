"""Training a scene end to end: what the reference spreads over code/train.py, Lightning's loop and MultiplyModel
(code/multiply_model.py) -- the two Adam optimisers and their schedule (:94-106, :219-225), the per-step choice between them
(:137-160), the stages at an epoch's end (:489-518), validation (:982-1131), the test run (:1183-1323) and Lightning's checkpoint
file -- on top of the stages this package already runs on the device.

Three layers, each usable alone:
  * pure host functions (no device, no library): step_plan, lr_at, epoch_end_plan, checkpoint_dict / split_checkpoint, and the
    record table of the optimiser launch (adam_table, access_mode);
  * DeviceAdam: torch.optim.Adam's arithmetic for every tensor of an optimiser in ONE launch (mp_adam_multi, csrc/optim.hip),
    with the learning rates, the step counts and a skip flag resident on the device;
  * Trainer: fit / validate / test over a scene folder.

The module imports without a device; the library is touched at the first DeviceAdam.step / Trainer call.
"""
import contextlib
import ctypes as C
import glob
import json
import os
from collections import Counter

import numpy as np
import torch

# ====================================================================================================================
# The schedule as pure host functions
# ====================================================================================================================
# the periods the reference hard-codes (multiply_model.py:491 mesh refresh, :509 mask refresh; train.py:31 validation, :20
# checkpoints) as config keys, and the defaults of init_params (:62-78)
SCHEDULE_DEFAULTS = dict(mesh_refresh_period=20, mask_refresh_period=50, validation_period=50, checkpoint_period=100,
                         depth_end=False, pose_start_epoch=200, pose_end_epoch=1000, pose_opt_interval=10, pose_opt_epoch=1,
                         depth_pose=False, depth_epoch=(), depth_cond_zero=False, it_per_loop=100, all_edge=False,
                         using_SAM=False, pose_correction_epoch=0, smpl_mesh_until_epoch=190, depth_frames=None)


def _cfg(cfg, key):
    v = cfg.get(key, None) if hasattr(cfg, "get") else getattr(cfg, key, None)
    return SCHEDULE_DEFAULTS[key] if v is None else v


def step_plan(epoch, cfg, has_sam_mask, is_certain):
    """What one training step does (multiply_model.py:137-160, :187-191, :195): which optimiser steps ('joint' | 'pose'), whether
    the four shape / colour network lists are frozen, whether the item's edge samples replace its samples, and whether the
    mesh-space terms (get_depth_order_loss) join the loss.  With using_SAM false the reference leaves cur_opt None and fails at
    :215; here that case takes the joint optimiser."""
    pose_epoch = epoch % _cfg(cfg, "pose_opt_interval")
    is_pose_depth_opt = bool(has_sam_mask and epoch >= _cfg(cfg, "pose_start_epoch") and pose_epoch < _cfg(cfg, "pose_opt_epoch")
                             and epoch < _cfg(cfg, "pose_end_epoch") and not _cfg(cfg, "depth_end"))
    optimizer, freeze, delayed = "joint", False, False
    if _cfg(cfg, "using_SAM"):
        delayed = bool(epoch < _cfg(cfg, "pose_correction_epoch") and not is_certain)
        if is_pose_depth_opt:
            optimizer = "pose"
        elif delayed:
            freeze = True
    return dict(optimizer=optimizer, freeze_shape=freeze, use_edge_samples=bool(delayed or _cfg(cfg, "all_edge")),
                mesh_losses=is_pose_depth_opt)


def lr_at(epoch, lr0, milestones, gamma):
    """torch.optim.lr_scheduler.MultiStepLR stepped once at every epoch's end (multiply_model.py:219-222): the rate in force
    DURING `epoch`.  The scheduler multiplies the running rate by gamma at each milestone, so this does too (not lr0 * gamma**k)."""
    lr = lr0
    for m, k in sorted(Counter(milestones).items()):
        if m <= epoch:
            lr = lr * gamma ** k
    return lr


def epoch_end_plan(epoch, cfg):
    """The stages after the last step of `epoch` (multiply_model.py:489-518)"""
    return dict(refresh_meshes=epoch != 0 and epoch % _cfg(cfg, "mesh_refresh_period") == 0,
                refresh_masks=epoch % _cfg(cfg, "mask_refresh_period") == 0,
                opt_depth=bool(_cfg(cfg, "depth_end")) and epoch in list(_cfg(cfg, "depth_epoch")))


# ====================================================================================================================
# Checkpoints: Lightning's layout (followed, not verified against a file Lightning wrote)
# ====================================================================================================================
def checkpoint_dict(epoch, global_step, model_state, body_states, optimizer_states, lr_schedulers, deterministic=None):
    """One torch.save dict: the scene model under 'model.', the body tables under 'body_model_list.<i>.<name>.weight'
    (MultiplyModel's attribute names), optimizer_states = [joint, pose].  deterministic (not None): recorded under 'deterministic'
    -- whether the run that wrote the checkpoint trained in the deterministic mode (train.deterministic)."""
    sd = {"model." + k: v for k, v in model_state.items()}
    for i, bs in enumerate(body_states):
        sd.update({f"body_model_list.{i}.{k}": v for k, v in bs.items()})
    ckpt = {"epoch": int(epoch), "global_step": int(global_step), "state_dict": sd, "optimizer_states": list(optimizer_states),
            "lr_schedulers": list(lr_schedulers)}
    if deterministic is not None:
        ckpt["deterministic"] = bool(deterministic)
    return ckpt


def deterministic_from_config(opt, default=None):
    """the config key `deterministic` (true / false; strings as the MP_TRAIN_DETERMINISTIC variable reads them) or `default`"""
    v = opt.get("deterministic", None) if hasattr(opt, "get") else getattr(opt, "deterministic", None)
    if v is None:
        return default
    from .train import _env_flag
    return _env_flag(v) if isinstance(v, str) else bool(v)


def split_checkpoint(ckpt):
    """-> (model state, [body table states]) of a checkpoint dict (one with only 'state_dict' is accepted)"""
    model, body = {}, {}
    for k, v in ckpt["state_dict"].items():
        if k.startswith("model."):
            model[k[len("model."):]] = v
        elif k.startswith("body_model_list."):
            i, name = k[len("body_model_list."):].split(".", 1)
            body.setdefault(int(i), {})[name] = v
        else:
            raise KeyError(f"unexpected checkpoint key {k!r}")
    return model, [body[i] for i in sorted(body)]


def scheduler_state(epoch, lr0s, milestones, gamma):
    """MultiStepLR.state_dict() after the step at the end of `epoch`"""
    last = epoch + 1
    return {"milestones": Counter(milestones), "gamma": gamma, "base_lrs": list(lr0s), "last_epoch": last, "verbose": False,
            "_step_count": last + 1, "_get_lr_called_within_step": False,
            "_last_lr": [lr_at(last, lr0, milestones, gamma) for lr0 in lr0s]}


def checkpoint_name(epoch, loss):
    """train.py:16-18: filename '{epoch:04d}-{loss}' as Lightning expands it"""
    return f"epoch={epoch:04d}-loss={loss}.ckpt"


def newest_checkpoint(folder="checkpoints"):
    """train.py:44"""
    found = sorted(glob.glob(os.path.join(folder, "epoch=*.ckpt")))
    return found[-1] if found else None


# ====================================================================================================================
# The optimiser launch
# ====================================================================================================================
ADAM_SCALAR, ADAM_VEC, ADAM_VEC_G4 = 0, 1, 2          # = include/multiply_hip.h
ADAM_BLOCK_ELEMS = 1024                               # elements one block covers per pass with 16-byte accesses (256 x 4)
ADAM_MAX_BLOCKS = 64                                  # per tensor; the rest of a larger tensor is strided over


class MpAdamDesc(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_void_p),
                ("n", C.c_longlong), ("group", C.c_int), ("block0", C.c_int), ("n_block", C.c_int), ("mode", C.c_int)]


def access_mode(p, g, m, v):
    """How mp_adam_multi may touch a tensor, from the four addresses: 16-byte accesses need p, m, v at the same offset within
    16 bytes (then a scalar head brings all three to a boundary); g joins them when it shares the offset, else it is read by
    dwords; anything else is the scalar path."""
    if not (p % 16 == m % 16 == v % 16) or p % 4:
        return ADAM_SCALAR
    if not g or g % 16 == p % 16:
        return ADAM_VEC
    return ADAM_VEC_G4


def adam_table(tensors, max_blocks=ADAM_MAX_BLOCKS):
    """tensors: [(p, g, m, v, step, n, group)] with addresses as ints (g 0 / None = inactive) -> (MpAdamDesc array,
    total_blocks).  Block ranges ascend from 0 and do not depend on g, so a step only rewrites g and mode (set_gradient)."""
    arr = (MpAdamDesc * max(len(tensors), 1))()
    block = 0
    for i, (p, g, m, v, step, n, group) in enumerate(tensors):
        nb = min(max(1, -(-int(n) // ADAM_BLOCK_ELEMS)), int(max_blocks))
        arr[i] = MpAdamDesc(p, g or None, m, v, step, int(n), int(group), block, nb, access_mode(p, g or 0, m, v))
        block += nb
    return arr, block


def set_gradient(rec, g):
    rec.g = g or None
    rec.mode = access_mode(rec.p, g or 0, rec.m, rec.v)


def _torch_adam_group_keys(lr, betas, eps):
    """the keys (and defaults) of a torch.optim.Adam param group of the installed torch, so that a saved state loads there"""
    g = dict(torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps).param_groups[0])
    g.pop("params")
    return g


class DeviceAdam:
    """torch.optim.Adam (no weight decay, no amsgrad) over param_groups = [{'params': [...], 'lr': float}, ...] with ONE launch
    per step.  exp_avg / exp_avg_sq live in two flat arenas (each tensor's slice at its parameter's offset within 16 bytes, so
    that the launch can use 16-byte accesses), the per-tensor step counts, the groups' learning rates and the record table are
    device-resident.  A parameter whose .grad is None is inactive for that step: nothing of it changes, its count stays."""
    STAGES = 4

    def __init__(self, param_groups, betas=(0.9, 0.999), eps=1e-8, max_blocks=ADAM_MAX_BLOCKS):
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.param_groups = []
        for g in param_groups:
            keys = _torch_adam_group_keys(float(g["lr"]), self.betas, self.eps)
            self.param_groups.append({"params": list(g["params"]), **keys})
        self.params = [p for g in self.param_groups for p in g["params"]]
        self.group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        assert self.params, "no parameters"
        dev = self.device = self.params[0].device
        offs, total = [], 0
        for p in self.params:
            assert p.dtype == torch.float32 and p.is_contiguous() and p.device == dev, "fp32 contiguous parameters on one device"
            total = (total + 3) // 4 * 4 + (p.data_ptr() % 16) // 4        # the parameter's offset within 16 bytes
            offs.append(total)
            total += p.numel()
        self.exp_avg = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total + 4, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(len(self.params), dtype=torch.float32, device=dev)
        self.lr = torch.tensor([float(g["lr"]) for g in self.param_groups], dtype=torch.float32, device=dev)
        self.offsets, self.max_blocks = offs, max_blocks
        self._table = None

    # ------------------------------------------------------------------ state
    def moments(self, i):
        o, n, shape = self.offsets[i], self.params[i].numel(), self.params[i].shape
        return self.exp_avg[o:o + n].view(shape), self.exp_avg_sq[o:o + n].view(shape)

    def set_lr(self, group, lr):
        """one asynchronous 4-byte device write; the table is not touched"""
        self.param_groups[group]["lr"] = float(lr)
        self.lr[group].fill_(float(lr))

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def state_dict(self):
        """torch.optim.Adam.state_dict()'s layout: state[i] only for parameters that have stepped (reads the counts)"""
        steps = self.steps.cpu()
        state = {}
        for i in range(len(self.params)):
            if float(steps[i]) > 0:
                m, v = self.moments(i)
                state[i] = {"step": self.steps[i].clone(), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        groups, k = [], 0
        for g in self.param_groups:
            n = len(g["params"])
            groups.append({**{key: val for key, val in g.items() if key != "params"}, "params": list(range(k, k + n))})
            k += n
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if [len(g["params"]) for g in groups] != [len(g["params"]) for g in self.param_groups]:
            raise ValueError("loaded state dict has different parameter groups")
        ids = [i for g in groups for i in g["params"]]
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.steps.zero_()
        for k, i in enumerate(ids):
            st = sd["state"].get(i)
            if st is None:
                continue
            m, v = self.moments(k)
            m.copy_(st["exp_avg"])
            v.copy_(st["exp_avg_sq"])
            self.steps[k:k + 1].copy_(torch.as_tensor(st["step"], dtype=torch.float32).reshape(1))
        for gi, g in enumerate(groups):
            self.set_lr(gi, g["lr"])
            b = tuple(float(x) for x in g.get("betas", self.betas))
            if b != self.betas or float(g.get("eps", self.eps)) != self.eps:
                raise ValueError("one betas / eps pair per DeviceAdam: the loaded groups carry another")

    # ------------------------------------------------------------------ the step
    def _build(self):
        recs = []
        for i, p in enumerate(self.params):
            m, v = self.moments(i)
            recs.append((p.data_ptr(), 0, m.data_ptr(), v.data_ptr(), self.steps.data_ptr() + 4 * i, p.numel(), self.group_of[i]))
        self._table, self.total_blocks = adam_table(recs, self.max_blocks)
        self._ptrs = [p.data_ptr() for p in self.params]
        nbytes = C.sizeof(self._table)
        self._table_dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        # pinned staging slots for the per-step refresh of the gradient pointers, reused only after their copy has run
        self._stage = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(self.STAGES)]
        self._stage_done = [None] * self.STAGES
        self._slot = 0

    def step(self, skip=None):
        """skip: a device bool / uint8 tensor of one element (e.g. torch.isnan(loss)): when set, the launch changes nothing.
        No host synchronisation: the table goes through pinned memory, the flag and the rates are read on the device."""
        from . import hip
        if self._table is None or self._ptrs != [p.data_ptr() for p in self.params]:
            self._build()
        for rec, p in zip(self._table, self.params):
            g = p.grad
            if g is not None:
                if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.device != self.device:
                    raise ValueError("DeviceAdam needs dense contiguous fp32 gradients on the parameters' device")
            set_gradient(rec, 0 if g is None else g.data_ptr())
        s = self._slot
        self._slot = (s + 1) % self.STAGES
        if self._stage_done[s] is not None:
            self._stage_done[s].synchronize()          # returns at once unless the host is STAGES steps ahead of the device
        C.memmove(self._stage[s].data_ptr(), C.addressof(self._table), C.sizeof(self._table))
        self._table_dev.copy_(self._stage[s], non_blocking=True)
        ev = self._stage_done[s] = self._stage_done[s] or torch.cuda.Event()
        ev.record()
        if skip is not None:
            assert skip.is_cuda and skip.numel() == 1 and skip.element_size() == 1, "skip: one device byte (bool / uint8)"
            skip = skip.reshape(1).view(torch.uint8)
        hip.lib().mp_adam_multi(self._table_dev, len(self.params), self.total_blocks, self.lr, skip, self.betas[0], self.betas[1],
                                self.eps, hip.stream())
        hip.invalidate_packed()


# ====================================================================================================================
# The trainer
# ====================================================================================================================
@contextlib.contextmanager
def _working_dir(path):
    """the run's folder as the working directory, as hydra makes it for the reference: the stage files and the datasets'
    stage_sam_mask lookup (datasets.Hi4DDataset._sam_mask) are relative to it"""
    os.makedirs(path, exist_ok=True)
    old = os.getcwd()
    os.chdir(path)
    try:
        yield
    finally:
        os.chdir(old)


def _batched(item, device):
    """an item with the batch dimension the reference's DataLoader(batch_size=1) adds, its tensors on the device (Lightning moves
    the batch there)"""
    def move(x):
        if torch.is_tensor(x):
            return x.to(device)
        if isinstance(x, dict):
            return {k: move(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return type(x)(move(v) for v in x)
        return x
    return move(torch.utils.data.default_collate([item]))


def _write_png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img).save(path)


def _to_u8(t):
    """(x * 255).astype(np.uint8) of the reference's writers, on values clipped to the byte range"""
    return (t.detach().float().clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()


def load_body_model_list(root, frame_ids, device):
    """multiply_model.py:44-51, :81-92: one BodyModelParams per person from the scene folder's mean_shape.npy (P,10), poses.npy
    (F,P,72) and normalize_trans.npy (F,P,3), rows of the training frames"""
    from .body_model_params import BodyModelParams
    shape = np.load(os.path.join(root, "mean_shape.npy"))
    poses = np.load(os.path.join(root, "poses.npy"))[list(frame_ids)]
    trans = np.load(os.path.join(root, "normalize_trans.npy"))[list(frame_ids)]
    out = []
    for p in range(shape.shape[0]):
        bm = BodyModelParams(len(frame_ids), model_type="smpl")
        f32 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
        bm.init_parameters("betas", f32(shape[None, p]))
        bm.init_parameters("global_orient", f32(poses[:, p, :3]))
        bm.init_parameters("body_pose", f32(poses[:, p, 3:]))
        bm.init_parameters("transl", f32(trans[:, p]))
        out.append(bm.to(device))
    return out


def build_trainer(scene_dir, out_dir, opt=None, dataset_opt=None, sam_predictor=None, smpl_tables=None, seed=42, log=print):
    """A Trainer over a scene folder (the layout datasets.Hi4DDataset reads): model, body tables, loss, the three datasets and --
    with a predictor -- the SAM server.  opt: the model config (default: the shipped one); dataset_opt: overrides of the dataset
    options (start_frame, end_frame, num_sample, pixel_per_batch, using_SAM, ...).  What code/train.py:37-40 and
    MultiplyModel.__init__ assemble."""
    from .config import load_config, to_config
    from .datasets import Hi4DDataset, Hi4DTestDataset, Hi4DValDataset
    from .loss import Loss
    from .multiply import Multiply
    opt = load_config() if opt is None else opt
    scene_dir = os.path.abspath(scene_dir)
    n_all = len(glob.glob(os.path.join(scene_dir, "image", "*.png")))
    base = dict(data_root=os.path.dirname(scene_dir), data_dir=os.path.basename(scene_dir), start_frame=0, end_frame=n_all,
                num_sample=512, pixel_per_batch=512, using_SAM=sam_predictor is not None)
    base.update(dataset_opt or {})
    frames = list(range(base["start_frame"], base["end_frame"]))
    opt.num_training_frames = len(frames)
    torch.manual_seed(seed)
    model = Multiply(opt, os.path.join(scene_dir, "mean_shape.npy"), smpl_tables=smpl_tables)
    dev = model.density.beta.device
    body = load_body_model_list(scene_dir, frames, dev)
    train_opt = to_config(base)
    full_opt = to_config(dict(base, num_sample=0))
    trainset = Hi4DDataset(train_opt, rng=np.random.RandomState(seed))
    validset = Hi4DValDataset(full_opt, rng=np.random.RandomState(seed + 1))
    testset = Hi4DTestDataset(full_opt)
    server = None
    if sam_predictor is not None:
        from .sam_prompts import SAMServer
        server = SAMServer(train_opt, predictor=sam_predictor)
    if opt.get("using_SAM", None) is None:
        opt.using_SAM = bool(base["using_SAM"])
    return Trainer(opt, model, body, Loss(opt.loss), trainset, validset, testset, sam_server=server, out_dir=out_dir, seed=seed,
                   log=log)


class Trainer:
    """fit / validate / test of one scene.  opt: the model config (learning_rate, sched_milestones, sched_factor, loss, and the
    keys of SCHEDULE_DEFAULTS); trainset: a datasets.Hi4DDataset (items, not a loader: an epoch visits every frame once in a
    shuffled order drawn from `rng`); validset / testset: Hi4DValDataset / Hi4DTestDataset or None; sam_server: a
    sam_prompts.SAMServer or None (the mask stage is then skipped and says so in the log).
    seed: every epoch re-seeds torch, the shuffle and the training set's sample draws from (seed, epoch), so that a run resumed from
    a checkpoint draws what the uninterrupted run draws (the reference seeds once, train.py:12, and a resumed run diverges).
    Config key `deterministic` (default: unset = the process default, MP_TRAIN_DETERMINISTIC): sets model.train_deterministic, the
    deterministic training mode (train.py); with it and a seed, a run resumed from a checkpoint reaches the SAME BITS
    as the uninterrupted run -- for steps whose plan carries no mesh-space term: get_depth_order_loss adds with torch scatters
    (index_add), which are outside the guarantee.  The mode a run trained in is recorded in its checkpoints ('deterministic')."""

    def __init__(self, opt, model, body_model_list, loss_fn, trainset, validset=None, testset=None, sam_server=None, out_dir=".",
                 rng=None, log=print, seed=None):
        self.opt, self.model, self.loss_fn = opt, model, loss_fn
        self.seed = seed
        self.body = list(body_model_list)
        self.trainset, self.validset, self.testset, self.sam_server = trainset, validset, testset, sam_server
        self.out_dir, self.log = os.path.abspath(out_dir), log
        self.rng = np.random.RandomState(0) if rng is None else rng
        self.cfg = dict(SCHEDULE_DEFAULTS)
        self.cfg.update({k: opt.get(k) for k in SCHEDULE_DEFAULTS if opt.get(k, None) is not None})
        self.last_depth_history = None
        det = deterministic_from_config(opt)
        if det is not None:
            model.train_deterministic = det
        if opt.get("using_SAM", None) is None:
            self.cfg["using_SAM"] = bool(getattr(trainset, "using_SAM", False))
        self.lr0, self.milestones, self.gamma = float(opt.learning_rate), list(opt.sched_milestones), float(opt.sched_factor)
        self.shape_nets = [model.foreground_implicit_network_list, model.foreground_rendering_network_list,
                           model.bg_implicit_network, model.bg_rendering_network]
        for bm in self.body:
            for name in bm.param_names:
                w = getattr(bm, name).weight
                w.data = w.data.contiguous()
                w.requires_grad = True                                            # multiply_model.py:49-51
        net_params = list(model.parameters())
        body_params = [p for bm in self.body for p in bm.parameters()]
        self.frozen_ids = {id(p) for nets in self.shape_nets for p in nets.parameters()}
        # multiply_model.py:94-106: two optimisers with separate states
        self.opt_joint = DeviceAdam([{"params": net_params, "lr": self.lr0}, {"params": body_params, "lr": 0.1 * self.lr0}],
                                    eps=1e-8)
        self.opt_pose = DeviceAdam([{"params": body_params, "lr": 0.1 * self.lr0}], eps=1e-8)
        self.optimizers = {"joint": self.opt_joint, "pose": self.opt_pose}
        self.epoch, self.global_step = 0, 0
        self._sums, self._n_steps = {}, 0
        self.last_epoch_log = None

    # ------------------------------------------------------------------ inputs
    def _device(self):
        return self.model.density.beta.device

    def _frame_index(self, idx):
        from . import hip
        return hip.device_ints([int(idx)], self._device()).reshape(1)

    def _body_inputs(self, inputs, idx, grad):
        from .mesh_losses import body_model_inputs
        fid = self._frame_index(idx)
        with torch.enable_grad() if grad else torch.no_grad():
            inputs["smpl_trans"], inputs["smpl_shape"], inputs["smpl_pose"] = body_model_inputs(self.body, fid)
        return fid

    def set_epoch_lr(self, epoch):
        for opt, bases in ((self.opt_joint, (self.lr0, 0.1 * self.lr0)), (self.opt_pose, (0.1 * self.lr0,))):
            for g, base in enumerate(bases):
                lr = lr_at(epoch, base, self.milestones, self.gamma)
                if opt.param_groups[g]["lr"] != lr:
                    opt.set_lr(g, lr)

    # ------------------------------------------------------------------ one step
    def training_step(self, item, epoch):
        """multiply_model.py:131-227 on one dataset item (inputs, targets) -> (plan, loss dict of device tensors)"""
        from .mesh_losses import body_model_inputs, get_depth_order_loss
        inputs, targets = _batched(item, self._device())
        idx = int(item[0]["idx"])
        plan = step_plan(epoch, self.cfg, "sam_mask" in inputs, bool(item[0].get("is_certain", True)))
        self.model.train()
        frozen = []
        if plan["freeze_shape"]:
            frozen = [p for nets in self.shape_nets for p in nets.parameters()]
            for p in frozen:
                p.requires_grad = False
        try:
            fid = self._body_inputs(inputs, idx, grad=True)
            with torch.no_grad():                                                  # :172-180
                _, _, inputs["smpl_pose_last"] = body_model_inputs(self.body, torch.clamp(fid - 1, min=0))
            inputs["current_epoch"] = epoch
            if plan["use_edge_samples"] and "edge_uv" in inputs:                   # :187-191
                inputs["uv"], targets["rgb"] = inputs["edge_uv"], targets["edge_rgb"]
                if "edge_sam_mask" in inputs:
                    inputs["sam_mask"] = inputs["edge_sam_mask"]
            out = self.model(inputs)
            lo = dict(self.loss_fn(out, targets))
            zero = torch.zeros(1, device=self._device())
            order, sil, inter = zero, zero, zero
            if plan["mesh_losses"]:                                                # :195-202
                order, sil, inter = get_depth_order_loss(self.model, inputs, epoch, loss_opt=self.opt.get("loss", None))
                lo["loss"] = lo["loss"] + inter.sum() + order.sum() + sil.sum()
            lo.update(depth_order_loss_pyrender=order, loss_instance_silhouette=sil, loss_interpenetration=inter)
            loss = lo["loss"]
            skip = torch.isnan(loss.detach()).reshape(-1)[:1]                      # :212-214 without the host round trip
            self.opt_joint.zero_grad()
            self.opt_pose.zero_grad()
            loss.sum().backward()
            for p in frozen:
                p.grad = None
            self.optimizers[plan["optimizer"]].step(skip=skip)
        finally:
            for p in frozen:
                p.requires_grad = True
        self.global_step += 1
        self._accumulate(lo, skip)
        return plan, lo

    def _accumulate(self, lo, skip):
        """device-side sums of the step's loss terms (one stacked vector); read once per epoch (epoch_log)"""
        keys = sorted(k for k, v in lo.items() if torch.is_tensor(v))
        vals = torch.cat([lo[k].detach().float().reshape(-1)[:1] for k in keys] + [skip.float()])
        vals = torch.where(skip, torch.cat([torch.zeros_like(vals[:-1]), vals[-1:]]), torch.nan_to_num(vals))
        if self._sums.get("keys") != keys:
            self._sums = {"keys": keys, "sum": vals}
        else:
            self._sums["sum"] = self._sums["sum"] + vals
        self._n_steps += 1

    def epoch_log(self, epoch):
        """the epoch's mean loss terms over the steps that were not skipped: ONE host read"""
        if not self._sums:
            return {"epoch": epoch, "steps": 0}
        keys, host = self._sums["keys"], self._sums["sum"].cpu().tolist()
        skipped = int(host[-1])
        n = max(self._n_steps - skipped, 1)
        out = {"epoch": epoch, "steps": self._n_steps, "skipped_nan": skipped, "global_step": self.global_step,
               "lr": self.opt_joint.param_groups[0]["lr"]}
        out.update({k: v / n for k, v in zip(keys, host)})
        self._sums, self._n_steps = {}, 0
        return out

    # ------------------------------------------------------------------ the stages at an epoch's end
    def _test_inputs(self, i):
        """frame i of the test set as one model input with the body tables' current rows"""
        inputs, targets, ppb, total, idx = self.testset[i]
        inputs, targets = _batched((inputs, targets), self._device())
        inputs["img_size"] = tuple(int(x) for x in targets["img_size"])
        self._body_inputs(inputs, idx, grad=False)
        return inputs, targets, int(ppb), int(total), int(idx)

    def refresh_masks(self, epoch):
        """get_instance_mask + get_sam_mask (multiply_model.py:741-939, :509-514): the files SAMServer.get_sam_mask reads, then
        the predictor rounds; the training set picks the new stage_sam_mask up at its next item"""
        from .mesh_losses import frame_instance_masks
        if self.sam_server is None:
            self.log(f"epoch {epoch}: instance-mask stage skipped: no sam_server was given")
            return None
        if self.testset is None:
            self.log(f"epoch {epoch}: instance-mask stage skipped: no test set to rasterise")
            return None
        self.model.eval()
        masks, kps = [], []
        for i in range(len(self.testset)):
            inputs, _, _, _, _ = self._test_inputs(i)
            m, _, kp = frame_instance_masks(self.model, inputs, use_smpl_mesh=epoch <= self.cfg["smpl_mesh_until_epoch"],
                                            res_up=self.opt.get("mask_res_up", 2))
            masks.append(m.cpu().numpy())
            kps.append(kp.cpu().numpy())
        dst = f"stage_instance_mask/{epoch:05d}"
        os.makedirs(dst, exist_ok=True)
        np.save(os.path.join(dst, "all_person_smpl_mask.npy"), np.stack(masks))
        np.save(os.path.join(dst, "2d_keypoint.npy"), np.stack(kps))
        return self.sam_server.get_sam_mask(epoch)

    def opt_depth(self, epoch):
        """multiply_model.py:230-486 over the test set (config key depth_frames: only those test items)"""
        from .datasets import draw_positions
        from .mesh_losses import opt_depth_frame
        if self.testset is None:
            self.log(f"epoch {epoch}: depth refinement skipped: no test set")
            return None
        ds = self.testset.dataset
        histories = []
        frames = self.opt.get("depth_frames", None)
        for i in (range(len(self.testset)) if frames is None else frames):
            inputs, targets, _, _, idx = self._test_inputs(i)
            if "org_sam_mask" not in inputs:
                self.log(f"epoch {epoch}: depth refinement skipped: the items carry no org_sam_mask")
                return None
            sam = inputs["org_sam_mask"][0]

            def sample_fn(idx=idx, sam=sam):
                pos, outside = draw_positions(ds.store.bbox[idx, 0], ds.store.bbox[idx, 1], ds.img_size, ds.num_sample or 512, ds.rng)
                rgb, uv, _, s = ds.store.sample(idx, pos, sam)
                return {"uv": uv[None], "index_outside": outside, "sam_mask": s[None]}, {"rgb": rgb[None]}

            histories.append(opt_depth_frame(self.model, self.body, self.loss_fn, inputs, sample_fn, epoch, self.cfg["it_per_loop"],
                                             self.lr0, loss_opt=self.opt.get("loss", None), depth_pose=self.cfg["depth_pose"],
                                             depth_cond_zero=self.cfg["depth_cond_zero"], res_up=self.opt.get("mask_res_up", 2)))
        return histories

    def training_epoch_end(self, epoch):
        from .mesh import refresh_canonical_meshes
        plan = epoch_end_plan(epoch, self.cfg)
        if plan["refresh_meshes"]:
            try:
                refresh_canonical_meshes(self.model, res_up=self.opt.get("mesh_res_up", 2))
            except Exception as e:              # :507-508: a level set that left the box; the old meshes stay
                self.log(f"epoch {epoch}: canonical mesh refresh failed, meshes kept: {e}")
        if plan["refresh_masks"]:
            self.refresh_masks(epoch)
        if plan["opt_depth"]:
            self.last_depth_history = self.opt_depth(epoch)
        return plan

    # ------------------------------------------------------------------ rendering a full frame
    def _render_frame(self, inputs, n_pixels, chunk, keys):
        """every view of the frame (all persons, each person alone) in chunks of `chunk` pixels -> {id: {key: (n_pixels, C)}}"""
        views = {}
        for s in range(0, n_pixels, chunk):
            part = dict(inputs, uv=inputs["uv"][:, s:s + chunk])
            for vid, out in self.model.render_views(part).items():
                for k in keys:
                    views.setdefault(vid, {}).setdefault(k, []).append(out[k].detach().reshape(min(chunk, n_pixels - s), -1))
        return {vid: {k: torch.cat(v, 0) for k, v in d.items()} for vid, d in views.items()}

    def _canonical_meshes(self, inputs, res_up):
        from .mesh import canonical_mesh
        return [canonical_mesh(self.model, p, cond=inputs["smpl_pose"][0, p, 3:] / np.pi, res_up=res_up)
                for p in range(self.model.num_person)]

    def validate(self, epoch):
        """multiply_model.py:982-1131: the canonical meshes and the three images per view of one validation frame"""
        inputs, targets = _batched(self.validset[0], self._device())
        self.model.eval()
        self._body_inputs(inputs, inputs["image_id"], grad=False)
        inputs["current_epoch"] = epoch
        H, W = (int(x) for x in targets["img_size"])
        for p, m in enumerate(self._canonical_meshes(inputs, self.opt.get("valid_res_up", 4))):
            os.makedirs("rendering", exist_ok=True)
            m.export(f"rendering/{epoch}_{p}.ply")
        n = H * W
        views = self._render_frame(inputs, n, min(int(targets["pixel_per_batch"]), n), ("rgb_values", "normal_values", "fg_rgb_values"))
        gt = targets["rgb"].reshape(H, W, 3)
        for vid, v in views.items():
            rgb = torch.cat([gt, v["rgb_values"].reshape(H, W, 3)], 0)              # ground truth above the prediction (:1104)
            _write_png(f"rendering/{epoch}_person{vid}.png", _to_u8(rgb))
            _write_png(f"normal/{epoch}_person{vid}.png", _to_u8((v["normal_values"].reshape(H, W, 3) + 1) / 2))
            _write_png(f"fg_rendering/{epoch}_person{vid}.png", _to_u8(v["fg_rgb_values"].reshape(H, W, 3)))
        return sorted(views)

    def test(self, frames=None):
        """multiply_model.py:1183-1323 for every test frame (or `frames`): test_mesh/<p>/%04d_{canonical,deformed}.ply and, per
        view id in (-1, 0 .. P-1), test_rendering / test_fg_rendering / test_normal / test_mask/<id>/%04d.png, plus
        test_instance_mask/<p>/%04d.png -- all of the frame's size (the reference stacks the ground truth above the rendering;
        here the rendering alone is written, which is what tools/eval_images.py compares).  With the config key test_overlay
        (default False) also test_overlay/%04d.png: the deformed meshes tinted per person over the input frame (_write_test_overlay).
        With test_mesh_cell (a cluster size in canonical units) or test_mesh_faces (a face count), both default None, each canonical
        mesh is simplified (ExtractedMesh.simplify) before its skinning weights are queried: both PLY files and the overlay then
        carry the reduced mesh."""
        from .mesh import ExtractedMesh
        from .mesh_losses import skinning
        with _working_dir(self.out_dir):
            self.model.eval()
            for i in (range(len(self.testset)) if frames is None else frames):
                inputs, targets, ppb, total, idx = self._test_inputs(i)
                H, W = (int(x) for x in targets["img_size"])
                meshes = self._canonical_meshes(inputs, self.opt.get("test_res_up", 4))
                cell, n_faces = self.opt.get("test_mesh_cell", None), self.opt.get("test_mesh_faces", None)
                if cell is not None or n_faces is not None:                        # both unset: the meshes as extracted
                    meshes = [m.simplify(cell=cell, target_faces=n_faces) for m in meshes]
                deformed = []
                for p, m in enumerate(meshes):
                    server, deformer = self.model.smpl_server_list[p], self.model.deformer_list[p]
                    so = server(inputs["smpl_params"][:, p, 0], inputs["smpl_trans"][:, p], inputs["smpl_pose"][:, p],
                                inputs["smpl_shape"][:, p])
                    deformer.K = 7                                                 # :1226-1229
                    try:
                        w = deformer.query_weights(m["vertices"])
                    finally:
                        deformer.K = 1
                    posed = skinning(m["vertices"][None], w, so["smpl_tfs"].reshape(1, 24, 4, 4))[0]
                    os.makedirs(f"test_mesh/{p}", exist_ok=True)
                    m.export(f"test_mesh/{p}/{idx:04d}_canonical.ply")
                    ExtractedMesh(posed, m["faces"]).export(f"test_mesh/{p}/{idx:04d}_deformed.ply")
                    deformed.append((posed, m["faces"]))
                if self.opt.get("test_overlay", False):
                    self._write_test_overlay(inputs, targets, deformed, idx)
                views = self._render_frame(inputs, total, min(ppb, total),
                                           ("rgb_values", "fg_rgb_values", "normal_values", "acc_map", "acc_person_list"))
                for vid, v in views.items():
                    _write_png(f"test_rendering/{vid}/{idx:04d}.png", _to_u8(v["rgb_values"].reshape(H, W, 3)))
                    _write_png(f"test_fg_rendering/{vid}/{idx:04d}.png", _to_u8(v["fg_rgb_values"].reshape(H, W, 3)))
                    _write_png(f"test_normal/{vid}/{idx:04d}.png", _to_u8((v["normal_values"].reshape(H, W, 3) + 1) / 2))
                    _write_png(f"test_mask/{vid}/{idx:04d}.png", _to_u8(v["acc_map"].reshape(H, W)))
                    if vid == -1:
                        inst = v["acc_person_list"].reshape(H, W, -1)
                        for p in range(inst.shape[2]):
                            _write_png(f"test_instance_mask/{p}/{idx:04d}.png", _to_u8(inst[:, :, p]))

    def _write_test_overlay(self, inputs, targets, deformed, idx):
        """test_overlay/%04d.png (the reference's ait_viewer_vis/vis_mesh_image.py): the frame's deformed meshes -- another
        topology per person, hence overlay.render_overlays' record table --, each tinted with its mesh_losses.COLOR_DICT colour,
        z-tested against each other and laid over the input frame with opacity 0.6, through the frame's own camera"""
        from . import overlay as OV
        from .mesh_losses import COLOR_DICT
        from .render import get_renderer
        H, W = (int(x) for x in targets["img_size"])
        cam = list(get_renderer(inputs)._cam16())
        scale = float(inputs["smpl_params"][0, 0, 0])                             # the renderer's units: get_renderer
        recs = []
        for p, (v, f) in enumerate(deformed):
            v = (v.detach().float() / scale).contiguous()
            tint = [c / 255.0 for c in COLOR_DICT[p % len(COLOR_DICT)]]
            recs.append((v, f, OV.vertex_colors(OV.vertex_normals(v, f), "tint", tint=tint)))
        frame = (targets["rgb"].reshape(1, H, W, 3).float() * 255).round().clamp(0, 255).to(torch.uint8)
        out = OV.render_overlays(recs, [0] * len(recs), cam, H, W, frames=frame, opacity=0.6)
        _write_png(f"test_overlay/{idx:04d}.png", out[0].cpu().numpy())

    # ------------------------------------------------------------------ checkpoints
    def checkpoint(self):
        """the checkpoint dict after the last finished epoch (self.epoch - 1)"""
        e = self.epoch - 1
        scheds = [scheduler_state(e, [self.lr0, 0.1 * self.lr0], self.milestones, self.gamma),
                  scheduler_state(e, [0.1 * self.lr0], self.milestones, self.gamma)]
        from .train import deterministic
        return checkpoint_dict(e, self.global_step, self.model.state_dict(), [bm.state_dict() for bm in self.body],
                               [self.opt_joint.state_dict(), self.opt_pose.state_dict()], scheds,
                               deterministic=deterministic(self.model))

    def save_checkpoint(self, path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(self.checkpoint(), path)
        return path

    def load_checkpoint(self, path):
        """a checkpoint of save_checkpoint, or any dict with 'state_dict' (then only the weights are restored)"""
        from . import hip
        ckpt = torch.load(path, map_location=self._device(), weights_only=False) if isinstance(path, (str, os.PathLike)) else path
        model_sd, body_sds = split_checkpoint(ckpt)
        with torch.no_grad():                                   # in place: the optimisers' tables keep their addresses
            own = self.model.state_dict()
            missing = [k for k in own if k not in model_sd]
            extra = [k for k in model_sd if k not in own]
            if missing or extra:
                raise KeyError(f"checkpoint / model mismatch: missing {missing[:4]}, unexpected {extra[:4]}")
            for k, v in own.items():
                v.copy_(model_sd[k])
            for bm, sd in zip(self.body, body_sds):
                for k, v in bm.state_dict().items():
                    v.copy_(sd[k])
        hip.invalidate_packed()
        if "optimizer_states" in ckpt:
            self.opt_joint.load_state_dict(ckpt["optimizer_states"][0])
            self.opt_pose.load_state_dict(ckpt["optimizer_states"][1])
        if "epoch" in ckpt:
            self.epoch, self.global_step = int(ckpt["epoch"]) + 1, int(ckpt.get("global_step", 0))
        return ckpt

    # ------------------------------------------------------------------ the loop
    def fit(self, max_epochs, resume=None):
        """epochs self.epoch .. max_epochs - 1.  resume: a checkpoint path, or True = the newest checkpoints/epoch=*.ckpt of the
        run folder (is_continue, train.py:42-45).  Returns the per-epoch logs."""
        logs = []
        with _working_dir(self.out_dir):
            if resume:
                path = newest_checkpoint() if resume is True else resume
                if path is None:
                    raise FileNotFoundError("resume: no checkpoints/epoch=*.ckpt in " + self.out_dir)
                self.load_checkpoint(path)
            for epoch in range(self.epoch, max_epochs):
                self.set_epoch_lr(epoch)
                if self.seed is not None:
                    torch.manual_seed(int(self.seed) * 100003 + epoch)
                    self.rng = np.random.RandomState((int(self.seed) * 100003 + epoch) % (1 << 32))
                    if hasattr(self.trainset, "rng"):
                        self.trainset.rng = np.random.RandomState((int(self.seed) * 100003 + epoch + 50021) % (1 << 32))
                for i in self.rng.permutation(len(self.trainset)):
                    self.training_step(self.trainset[int(i)], epoch)
                self.training_epoch_end(epoch)
                if self.validset is not None and (epoch + 1) % self.cfg["validation_period"] == 0:
                    self.validate(epoch)
                self.epoch = epoch + 1
                log = self.last_epoch_log = self.epoch_log(epoch)
                logs.append(log)
                self.log(json.dumps(log))
                if (epoch + 1) % self.cfg["checkpoint_period"] == 0:
                    self.save_checkpoint(os.path.join("checkpoints", checkpoint_name(epoch, log.get("loss", float("nan")))))
                    self.save_checkpoint(os.path.join("checkpoints", "last.ckpt"))
            self.set_epoch_lr(self.epoch)
        return logs
