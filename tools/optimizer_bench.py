#!/usr/bin/env python
"""DeviceAdam.step (mp_adam_multi, one launch + the count launch) against torch.optim.Adam(fused=True).step() on the parameter set
and one real gradient of the shipped 2-person model, alternating in one process.
    python tools/optimizer_bench.py [--reps 50] [--rounds 5]
Each round times `reps` steps of one optimiser, then of the other, between device events (GPU time of the enqueued work) and with
the host clock (time until the calls return, then the final synchronize); the order within a round alternates.  Both optimisers
own a copy of the parameters; the gradient tensors are the training step's own (views of the flat per-iteration buffer)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
args, sys.argv = ap.parse_args(), sys.argv[:1]

import bench  # noqa: E402
from multiply_amd.config import load_config  # noqa: E402
from multiply_amd.loss import Loss  # noqa: E402
from multiply_amd.trainer import DeviceAdam  # noqa: E402

model, inp, tables, sc = bench.build_model(128, seed=0)
gin = bench.to_dev(inp)
model.train()
g = torch.Generator().manual_seed(0)
sel = torch.randperm(gin["uv"].shape[1], generator=g)[:512].cuda()
tin = dict(gin, uv=gin["uv"][:, sel].contiguous(), current_epoch=301, index_outside=torch.zeros(512, dtype=torch.bool, device="cuda"),
           smpl_pose_last=gin["smpl_pose"] + 0.01)
loss = Loss(load_config().loss)(model(tin), {"rgb": torch.rand(1, 512, 3, generator=g).cuda()})["loss"]
loss.backward()
params = [p for p in model.parameters() if p.grad is not None]
grads = [p.grad for p in params]
n_el = sum(p.numel() for p in params)
copies = {}
for name in ("device", "torch"):
    ps = [p.detach().clone().requires_grad_(True) for p in params]
    for q, gr in zip(ps, grads):
        q.grad = gr
    copies[name] = ps
opts = {"device": DeviceAdam([{"params": copies["device"], "lr": 5e-4}], eps=1e-8),
        "torch": torch.optim.Adam(copies["torch"], lr=5e-4, eps=1e-8, fused=True)}


def timed(opt, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        opt.step()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (t1 - t0) * 1e6 / reps


for opt in opts.values():
    timed(opt, 5)
res = {k: {"gpu_us": [], "host_us": []} for k in opts}
for r in range(args.rounds):
    for name in (("device", "torch") if r % 2 == 0 else ("torch", "device")):
        gpu, host = timed(opts[name], args.reps)
        res[name]["gpu_us"].append(round(gpu, 2))
        res[name]["host_us"].append(round(host, 2))
med = lambda v: sorted(v)[len(v) // 2]
diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(copies["device"], copies["torch"]))
print(json.dumps({"tensors": len(params), "elements": n_el, "reps": args.reps, "rounds": args.rounds,
                  "device_adam": res["device"], "torch_fused_adam": res["torch"],
                  "median_gpu_us": {k: med(v["gpu_us"]) for k, v in res.items()},
                  "median_host_us": {k: med(v["host_us"]) for k, v in res.items()},
                  "bytes_per_step": 28 * n_el, "max_abs_param_difference_after_all_steps": diff}))
