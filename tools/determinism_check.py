#!/usr/bin/env python
"""GPU box: is the rendered frame a function of the library alone?  `save` renders bench.py's headline frame twice (compares the two
renders bit for bit) and stores the outputs; `cmp` renders it again -- in another process, possibly with another library through
MP_LIB_PATH (another cluster layout, another point-to-wave mapping: tools/ab_build.sh) -- and counts the elements that differ.
    python tools/determinism_check.py save;  MP_LIB_PATH=... python tools/determinism_check.py cmp        (profiles/r06_determinism.txt)
`train`: is a training step a function of its inputs?  bench.py's training step (512 rays, epoch 301; --pose-grad: the body inputs
require grad) runs twice from the same state and the same seed -- forward, loss, backward, no optimiser step -- and every gradient
tensor is compared: how many elements differ and by how much.  --deterministic: in the deterministic training mode
(model.train_deterministic), where every count must be 0.
    python tools/determinism_check.py train [--deterministic] [--pose-grad]                      (profiles/deterministic_train.txt)"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mode = sys.argv[1]
flags = sys.argv[2:]
sys.argv = sys.argv[:1]
import bench


def train_mode():
    import contextlib
    from multiply_amd import train as T
    from multiply_amd.config import load_config
    from multiply_amd.loss import Loss
    model, inp, tables, sc = bench.build_model(128, seed=0)
    model.convergence_group = 512
    model.train_deterministic = "--deterministic" in flags
    gin = bench.to_dev(inp)
    body = ("smpl_pose", "smpl_trans", "smpl_shape") if "--pose-grad" in flags else ()
    for k in body:
        gin[k] = gin[k].detach().clone().requires_grad_(True)
    g = torch.Generator(device="cpu").manual_seed(0)
    R = gin["uv"].shape[1]
    sel = torch.randperm(R, generator=g)[:512].cuda()
    tin = dict(gin, uv=gin["uv"][:, sel].contiguous(), current_epoch=301, index_outside=torch.zeros(512, dtype=torch.bool, device="cuda"),
               smpl_pose_last=gin["smpl_pose"].detach() + 0.01)
    gt = {"rgb": torch.rand(1, 512, 3, generator=g).cuda()}
    loss_fn = Loss(load_config().loss)
    model.train()
    runs = []
    for _ in range(2):
        torch.manual_seed(7)                                  # the step's own draws (train.make_draws)
        model.zero_grad(set_to_none=True)
        for k in body:
            gin[k].grad = None
        out = model(tin)
        with contextlib.redirect_stdout(sys.stderr):
            lo = loss_fn(out, gt)
        lo["loss"].backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        grads.update({k: gin[k].grad.detach().clone() for k in body})
        grads["loss"] = lo["loss"].detach().clone().reshape(-1)
        runs.append(grads)
    a, b = runs
    print(f"training step twice from the same state: deterministic mode {T.deterministic(model)}, pose_grad {bool(body)}, "
          f"precision {T.TRAIN_PRECISION}, workspace {T.det_workspace_bytes()} bytes")
    n_diff = n_all = 0
    worst = 0.0
    for k in a:
        d = (a[k].double() - b[k].double()).abs().nan_to_num()
        nd = int((d > 0).sum())
        n_diff += nd
        n_all += d.numel()
        rel = float(d.max() / (a[k].double().abs().max() + 1e-300))
        worst = max(worst, rel)
        if nd or k == "loss":
            print(f"{k:64s} differing {nd:8d} of {d.numel():8d}   max |diff| {float(d.max()):.3e}   relative to the tensor's max {rel:.3e}")
    print(f"total: {n_diff} of {n_all} elements of {len(a)} tensors differ; worst relative difference {worst:.3e}")


if mode == "train":
    train_mode()
    sys.exit(0)
model, inp, tables, sc = bench.build_model(128)
model.convergence_group = 512
with torch.no_grad():
    out = model(bench.to_dev(inp))
    torch.cuda.synchronize()
    out2 = model(bench.to_dev(inp))
    torch.cuda.synchronize()
keys = ("rgb_values", "acc_map", "acc_person_list", "normal_values", "fg_rgb_values")
cur = {k: out[k].detach().cpu() for k in keys}
print("same process, second render:", {k: float((cur[k] - out2[k].detach().cpu()).abs().nan_to_num().max()) for k in keys})
if mode == "save":
    torch.save(cur, "/tmp/det_ref.pt")
else:
    ref = torch.load("/tmp/det_ref.pt")
    for k in keys:
        d = (cur[k].double() - ref[k].double()).abs().nan_to_num()
        print(f"{k:18s} max {float(d.max()):.3e} mean {float(d.mean()):.3e} differing elements {int((d > 0).sum())} of {d.numel()}")
