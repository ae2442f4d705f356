#!/usr/bin/env python
"""Times the keypoint fit of one frame (P persons, `--iters` Adam steps, the coco25 map) two ways on the same inputs:

  fused     keypoint_fit.refine_frame: ONE launch of mp_kp_fit for all persons and steps
  autograd  the loop as it has to be written without it: per person SMPLServer.forward under autograd (full 6890-vertex body,
            mp_smpl_pose + its adjoint), the keypoints, projection and loss in torch, torch.optim.Adam with the reference's
            three parameter groups, one step after the other

Times are device events around `--reps` repetitions after `--warmup` (the two ways alternate, repetition by repetition), reported
as the median and the spread per frame and per person-frame; the two results are compared so that faster is not different.
`--mode fused|autograd` runs one way only and without timing events: for a `rocprofv3 --kernel-trace --stats` run of its own, whose
kernel rows give the launches per frame and mp_kp_fit's time per Adam step.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_inputs(P, seed):
    from multiply_amd import keypoint_fit as KF
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_smpl_tables
    server = SMPLServer(smpl_tables=make_smpl_tables(0))
    kmap = KF.KeypointMap.coco25()
    g = torch.Generator().manual_seed(seed)
    gt = torch.zeros(P, 85)
    gt[:, 0] = torch.linspace(-0.5, 0.5, P) if P > 1 else 0.0
    gt[:, 2] = 3.0
    gt[:, 3:75] = 0.25 * torch.randn(P, 72, generator=g)
    gt[:, 75:] = 0.5 * torch.randn(P, 10, generator=g)
    cam = {"fx": 500.0, "fy": 500.0, "cx": 256.0, "cy": 256.0}
    pack = kmap.pack([server] * P)
    uv, _ = KF.project_keypoints([server] * P, gt, kmap, cam, pack=pack)
    start = gt.clone()
    start[:, 3:75] += 0.1 * torch.randn(P, 72, generator=g)
    start[:, 0:3] += 0.03 * torch.randn(P, 3, generator=g)
    c = KF.keypoint_weights(torch.full((P, kmap.K), 0.9), kmap, 0.6)
    return dict(server=server, kmap=kmap, pack=pack, cam=cam, targets=uv.contiguous(), c=c.cuda(), start=start.cuda(),
                prev=start[:, :75].cuda().contiguous())


def run_fused(inp, iters):
    from multiply_amd import keypoint_fit as KF
    P = inp["start"].shape[0]
    return KF.refine_frame([inp["server"]] * P, inp["start"], inp["targets"], inp["c"], inp["cam"], inp["kmap"], prev=inp["prev"],
                           iters=iters, lr=1e-3, pack=inp["pack"])["params"]


def run_autograd(inp, iters):
    """the reference's loop (preprocessing_multiple_trace.py:425-485) on SMPLServer.forward"""
    from multiply_amd import keypoint_fit as KF
    server, kmap = inp["server"], inp["kmap"]
    dev = inp["start"].device
    M = torch.from_numpy(kmap.dense()).float().to(dev)
    sv = torch.from_numpy(kmap.support).to(dev)
    fx, fy, cx, cy = (inp["cam"][k] for k in ("fx", "fy", "cx", "cy"))
    one = torch.ones(1, device=dev)
    out = []

    def rot6d(th):                                   # first two columns of Rodrigues' matrix (rotation.py axis_to_rot6D)
        th = th.reshape(24, 3)
        ang = (th + 1e-8).norm(dim=1, keepdim=True)
        n = th / ang
        z = torch.zeros_like(n[:, 0])
        Km = torch.stack([z, -n[:, 2], n[:, 1], n[:, 2], z, -n[:, 0], -n[:, 1], n[:, 0], z], 1).reshape(24, 3, 3)
        Rm = torch.eye(3, device=dev) + torch.sin(ang)[:, :, None] * Km + (1 - torch.cos(ang))[:, :, None] * (Km @ Km)
        return Rm[:, :, :2]

    for q in range(inp["start"].shape[0]):
        pose, trans, betas = (x.clone().requires_grad_(True) for x in KF.split_params(inp["start"][q]))
        opt = torch.optim.Adam([{"params": betas, "lr": 1e-3}, {"params": pose, "lr": 1e-3}, {"params": trans, "lr": 1e-3}],
                               lr=2e-3, betas=(0.9, 0.999))
        prev_t, prev_6d = inp["prev"][q, :3], rot6d(inp["prev"][q, 3:75]).detach()
        for _ in range(iters):
            opt.zero_grad()
            body = server(one, trans, pose, betas)
            src = torch.cat([body["smpl_jnts"][0], body["smpl_verts"][0][sv]], 0)
            X = M @ src
            uv = torch.stack([fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy], 1)
            r2 = (inp["targets"][q] - uv) ** 2
            l2d = (inp["c"][q][:, None] * (1e4 * r2 / (r2 + 1e4))).sum()
            lt = 5.0 * ((rot6d(pose) - prev_6d) ** 2).mean() + ((trans - prev_t) ** 2).mean()
            (1e-2 * l2d + 6.0 * lt).backward()
            opt.step()
        out.append(KF.pack_params(pose.detach(), trans.detach(), betas.detach()))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--persons", type=int, default=2)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mode", choices=("both", "fused", "autograd"), default="both")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from multiply_amd import hip
    hip.require_device()
    inp = make_inputs(a.persons, a.seed)
    ways = {"fused": run_fused, "autograd": run_autograd}
    if a.mode != "both":
        for _ in range(a.reps):
            ways[a.mode](inp, a.iters)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "keypoint_fit_bench", "mode": a.mode, "persons": a.persons, "iters": a.iters, "frames": a.reps}))
        return
    for _ in range(a.warmup):
        res = {k: f(inp, a.iters) for k, f in ways.items()}
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    for _ in range(a.reps):
        for k, f in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res[k] = f(inp, a.iters)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out = {"tool": "keypoint_fit_bench", "persons": a.persons, "iters": a.iters, "reps": a.reps, "keypoints": inp["kmap"].K,
           "support_vertices": inp["kmap"].S}
    for k, v in ms.items():
        out[k] = {"ms_per_frame_median": statistics.median(v), "ms_per_frame_min": min(v), "ms_per_frame_max": max(v),
                  "ms_per_person_frame": statistics.median(v) / a.persons,
                  "us_per_adam_step_per_person": 1e3 * statistics.median(v) / a.persons / max(a.iters, 1)}
    out["speedup_median"] = out["autograd"]["ms_per_frame_median"] / out["fused"]["ms_per_frame_median"]
    out["max_abs_param_difference"] = float((res["fused"] - res["autograd"]).abs().max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
