#!/usr/bin/env python
"""Training iterations only (bench.py's train_iter leg): ms/iter, GPU phase times; run it under
`rocprofv3 --kernel-trace` + tools/rocpd_summary.py for the per-kernel table of ONE iteration's work.
    python tools/train_bench.py [steps] [warmup] [--epoch E] [--mesh-index auto|index|brute] [--pose-grad] [--train-geometry]
                                                   [--train-interpenetration] [--deterministic]
--epoch E: every forward sees current_epoch = E instead of bench.py's 301.  Below 250 the in / off-surface flags are on; as the
trainer has refreshed the canonical meshes by then (every 20 epochs), they are extracted once before the loop.
--mesh-index: model.mesh_index_mode (the flags' signed distance through the face index or by brute force).
--pose-grad: smpl_pose / smpl_trans / smpl_shape require grad (the reference optimises them in every step), and the iteration is
timed once per MP_SDF_POSE_GRAD_MODE ('layerwise', 'fused'), each in a fresh child process of this one, back to back on the same
device; every line names the SDF evaluator class in use.  As in the trainer, the previous frame's pose enters the temporal term as
a constant and the three inputs' gradients are cleared before every forward.
--train-geometry: model.train_geometry = True, and the sum of depth_person_solo_level_list joins the timed loss (through the
temporal term, which the loss adds with weight 1), so that the iteration holds both extra launches: mp_composite_geometry in the
forward and mp_tr_composite_geometry_bwd in the backward.
--train-interpenetration: model.train_interpenetration = True, and the term joins the timed loss the same way: the probe, the
partners' SDF at the probed points and mp_pen_loss in the forward (with the term's one host read of the pair counts) and, with
--pose-grad, its adjoint (mp_tf_sdf_bwd / _dx per partner, mp_tr_warp_bwd, mp_pen_scatter_bwd) at the head of the backward.
--deterministic: model.train_deterministic = True (the deterministic training mode); the line then also reports the
bytes of the contractions' workspace."""
import json
import os
import subprocess
import sys

if "--pose-grad" in sys.argv[1:]:            # the parent: starts one child per mode and never touches the device itself
    rest = [a for a in sys.argv[1:] if a != "--pose-grad"]
    res = {}
    for mode in ("layerwise", "fused"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + rest + ["--pose-grad-child"], stdout=subprocess.PIPE, text=True,
                           env=dict(os.environ, MP_SDF_POSE_GRAD_MODE=mode))
        sys.stdout.write(r.stdout)
        if r.returncode != 0:
            sys.exit(f"the {mode!r} run failed with status {r.returncode}")
        res[mode] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    lw, fu = res["layerwise"]["ms_per_iter"], res["fused"]["ms_per_iter"]
    print(f"pose-optimising iteration: layerwise {lw:.3f} ms ({res['layerwise']['sdf_evaluator']}), fused {fu:.3f} ms "
          f"({res['fused']['sdf_evaluator']}): {lw - fu:+.3f} ms, x{lw / fu:.3f}")
    sys.exit(0)

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.argv, args = sys.argv[:1], sys.argv[1:]
opts = {}
POSE_GRAD = "--pose-grad-child" in args
TRAIN_GEOMETRY = "--train-geometry" in args
TRAIN_PEN = "--train-interpenetration" in args
DETERMINISTIC = "--deterministic" in args
if DETERMINISTIC:
    args.remove("--deterministic")
if TRAIN_GEOMETRY:
    args.remove("--train-geometry")
if TRAIN_PEN:
    args.remove("--train-interpenetration")
if POSE_GRAD:
    args.remove("--pose-grad-child")
for flag in ("--epoch", "--mesh-index"):
    if flag in args:
        i = args.index(flag)
        opts[flag] = args[i + 1]
        del args[i:i + 2]
import bench   # noqa: E402

steps = int(args[0]) if args else 20
warm = int(args[1]) if len(args) > 1 else 3
model, inp, tables, sc = bench.build_model(128, seed=0)
model.convergence_group = 512
gin = bench.to_dev(inp)
if POSE_GRAD:
    BODY = ("smpl_pose", "smpl_trans", "smpl_shape")
    for k in BODY:
        gin[k] = gin[k].detach().clone().requires_grad_(True)

    def _as_the_trainer(mod, a):
        """the trainer's optimiser clears the body parameters' gradients every step, and the previous frame's pose is a constant
        (bench.train_iterations derives it from the tensor that now requires grad: the temporal term would cancel)"""
        for k in BODY:
            gin[k].grad = None
        return (dict(a[0], smpl_pose_last=a[0]["smpl_pose_last"].detach()),) + tuple(a[1:])
    model.register_forward_pre_hook(_as_the_trainer)
if TRAIN_GEOMETRY:
    model.train_geometry = True
    model.register_forward_hook(lambda mod, a, out: {**out, "temporal_loss": out["temporal_loss"] + out["depth_person_solo_level_list"].sum()}
                                if mod.training else None)
if TRAIN_PEN:
    model.train_interpenetration = True
    model.register_forward_hook(lambda mod, a, out: {**out, "temporal_loss": out["temporal_loss"] + out["interpenetration_loss"].sum()}
                                if mod.training else None)
if DETERMINISTIC:
    model.train_deterministic = True
if "--mesh-index" in opts:
    model.mesh_index_mode = opts["--mesh-index"]
EPOCH = int(opts.get("--epoch", 301))
if EPOCH != 301:
    if EPOCH < 250:
        from multiply_amd.mesh import refresh_canonical_meshes
        refresh_canonical_meshes(model)
        print("canonical meshes:", [int(t.shape[1]) for t in model.mesh_face_vertices_list], "faces; mesh_index_mode", model.mesh_index_mode)
    model.register_forward_pre_hook(lambda mod, a: (dict(a[0], current_epoch=EPOCH),) + tuple(a[1:]))


def barrier():
    torch.cuda.synchronize()


dt, ph, loss, stats, host_ms = bench.train_iterations(model, gin, steps, warm, False, barrier, seed=0, rays=512)
from multiply_amd import train as T
extra = {"deterministic": T.deterministic(model), "det_workspace_bytes": T.det_workspace_bytes()}
if POSE_GRAD:
    graph = model._last_train
    assert graph.pose_grad
    extra.update({"pose_grad": True, "sdf_pose_grad_mode": T.SDF_POSE_GRAD_MODE,
                  "sdf_evaluator": "/".join(sorted({type(f["it"]).__name__ for f in graph.fg.values()}))})
print(json.dumps({**extra, "train_geometry": TRAIN_GEOMETRY, "train_interpenetration": TRAIN_PEN, "current_epoch": EPOCH, "mesh_index_mode": model.mesh_index_mode, "ms_per_iter": 1e3 * dt / steps, "host_ms_per_iter": host_ms, "gpu_ms": {"forward+loss": ph[0], "backward": ph[1], "allreduce": ph[2],
                                                               "adam": ph[3]}, "hit_rays": stats["n_hit"], "loss": loss}))

if POSE_GRAD:
    sys.exit(0)

# ---- host-side view: how long does the HOST need to enqueue each part (it runs ahead of the GPU unless something syncs)?
import time
from multiply_amd.config import load_config
from multiply_amd.loss import Loss
model.train()
loss_fn = Loss(load_config().loss)
opt = torch.optim.Adam(model.parameters(), lr=5e-4, fused=True)
g = torch.Generator().manual_seed(0)
R = gin["uv"].shape[1]
acc = {"fwd": 0.0, "loss": 0.0, "bwd": 0.0, "adam": 0.0, "sync": 0.0}
model.async_setup = os.environ.get('MP_ASYNC_SETUP', '1') == '1'
n = 10
for it in range(n + 2):
    sel = torch.randperm(R, generator=g)[:512].cuda()
    tin = dict(gin); tin["uv"] = gin["uv"][:, sel].contiguous()
    tin.update(current_epoch=EPOCH, index_outside=torch.zeros(512, dtype=torch.bool, device="cuda"), smpl_pose_last=gin["smpl_pose"] + 0.01)
    gt = {"rgb": torch.rand(1, 512, 3, generator=g).cuda()}
    torch.cuda.synchronize()
    t0 = time.perf_counter(); out = model(tin)
    t1 = time.perf_counter(); lo = loss_fn(out, gt)
    t2 = time.perf_counter(); opt.zero_grad(set_to_none=True); lo["loss"].backward()
    t3 = time.perf_counter(); opt.step()
    t4 = time.perf_counter(); torch.cuda.synchronize()
    t5 = time.perf_counter()
    if it >= 2:
        for k, d in zip(acc, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4)):
            acc[k] += 1e3 * d / n
print("host ms per iteration until each call RETURNS (then the final synchronize):", {k: round(v, 2) for k, v in acc.items()})
