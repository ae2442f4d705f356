#!/usr/bin/env python
"""What the registration's own kernels cost beside the closest queries they sit between.
    python tools/registration_bench.py [--out profiles/registration.txt] [--reps 30] [--samples 100000]
synthetic.closed_body_mesh against a rotated, shifted copy of itself, `samples` surface samples per side.  HIP events around the
launches of one ICP iteration, median (min .. max) of `reps` after 5 warm-ups (the protocol of profiles/mesh_closest.txt), split
into the two closest queries -- the yardstick: what the library could already time before the registration existed -- and
apply + rows + step, the new kernels.  Then iterations to convergence and the wall time of one registration.register call, reading
the state back every 5 iterations against every iteration."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--samples", type=int, default=100_000)
args = ap.parse_args()
sys.argv = sys.argv[:1]
import bench  # noqa: E402
from multiply_amd import hip, metrics, registration as reg  # noqa: E402
from multiply_amd.synthetic import closed_body_mesh  # noqa: E402

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, before=None, reps=args.reps, warm=5):
    ts = []
    for k in range(warm + reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f}) us"

torch.cuda.set_device(0)
hip.require_device()
model, inp, tables, sc = bench.build_model(128, seed=0)
bv, bf = closed_body_mesh(model.smpl_server_list[0])
axis = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
th = np.deg2rad(10.0)
T0 = reg.Similarity(1.0, np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K, [0.03, -0.02, 0.025])
dv = T0.apply(bv.double()).float().contiguous()
n = args.samples
say(f"Point-to-plane registration beside its closest queries.  {torch.cuda.get_device_name(0)}, one device, one session; library "
    f"{hip.lib_source_sha16()}")
say(f"closed_body_mesh ({bf.shape[0]} faces) onto its copy under 10 degrees about (1, 2, -1) and t = (0.03, -0.02, 0.025); {n} samples "
    f"per side; 'auto' face index.  HIP events, median (min .. max) of {args.reps} after 5 warm-ups.")
say()

details = {}
T, info = reg.register((bv, bf), (dv, bf), kind="rigid", n_samples=n, details=details)
err = float((torch.from_numpy(T.apply(bv.cpu().numpy().astype(np.float64))) - torch.from_numpy(T0.apply(bv.cpu().numpy().astype(np.float64)))).abs().max())
say(f"register(rigid, centroid start): {info['iterations']} iterations, converged {info['converged']}, rms {info['rms']:.3e}, "
    f"max_v |T v - T0 v| = {err:.3e}")
fr = details["frames"][0]
S, D = fr["src"], fr["dst"]
slots = torch.zeros(2, hip.REG_SLOT, dtype=torch.float64, device="cuda")
work, x = hip.reg_work("cuda"), torch.empty(n, 3, device="cuda")
for tag, st_np in (("first iteration (the centroid start)", details["iterations"][0]["state_before"]),
                   ("last iteration (converged)", details["iterations"][-1]["state_before"])):
    st0 = torch.from_numpy(st_np.copy()).cuda()
    st0[hip.REG_FLAG] = 0.0
    state = st0.clone()
    xs, xd = hip.reg_apply(S["pts"], state), hip.reg_apply(D["pts"], state, inverse=True)
    _, f1, q1 = hip.mesh_closest(xs, D["fv"], index=D["index"])
    _, f2, p2 = hip.mesh_closest(xd, S["fv"], index=S["index"])

    def queries():
        hip.mesh_closest(xs, D["fv"], index=D["index"])
        hip.mesh_closest(xd, S["fv"], index=S["index"])

    def ours():
        hip.reg_apply(S["pts"], state, out=x)
        hip.reg_rows(S["pts"], q1, D["fn"], state, slots[0], face=f1, work=work)
        hip.reg_apply(D["pts"], state, inverse=True, out=x)
        hip.reg_rows(p2, D["pts"], S["fn"], state, slots[1], face=f2, normals_in_source=True, work=work)
        hip.reg_step(slots, state, similarity=False, reject=3.0, tol=0.0)

    tq, to = timed(queries), timed(ours, before=lambda: state.copy_(st0))
    say(f"{tag}:")
    say(f"    the two closest queries (yardstick)       {fmt(tq)}")
    say(f"    2 x apply + 2 x rows + step (new kernels)  {fmt(to)}   = {100 * to[0] / (to[0] + tq[0]):.1f} % of the iteration")
say()


def wall(check_every, reps=5):
    ts = []
    for k in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        _, i = reg.register((bv, bf), (dv, bf), kind="rigid", n_samples=n, check_every=check_every)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:]), i


for ce in (5, 1):
    md, lo, hi, i = wall(ce)
    say(f"one register() call, state read back every {ce} iteration(s): {md:8.2f} ({lo:.2f} .. {hi:.2f}) ms wall, median of 5 after 1 "
        f"warm-up; {i['iterations']} iterations taken, {len(i['history'])} read-backs (sampling and the two index builds included)")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
