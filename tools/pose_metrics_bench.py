#!/usr/bin/env python
"""Times the posing of a whole sequence's bodies and their scoring (multiply_amd/pose_metrics.py): F frames of P persons,
prediction and ground truth = 2 F P parameter rows (1 200 by default), on the synthetic body tables.
    python tools/pose_metrics_bench.py [--frames 300] [--persons 2] [--rounds 5] [--window-ms 350]
Three things: the loop it replaces -- one SMPLServer.pose_into call per row --, ONE SMPLServer.pose_batch call of the same rows, and
the whole pose_metrics call (posing both sequences per person, six means per item, the depth relations; a host clock around it,
since it ends with the results on the host).  Device events around windows of back-to-back calls of about a third of a second each,
after a warm-up; the variants take turns within each of five rounds (ms per call, sorted); bytes and launches are counted from the shapes.  The text it prints is what profiles/pose_metrics.txt holds."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, reps, host=False):
    """ms per call of `reps` back-to-back calls: device events around them, or (host) a host clock between two synchronisations"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return ((time.perf_counter() - t0) * 1e3 if host else e0.elapsed_time(e1)) / reps


def alternated(variants, rounds):
    """variants: (name, fn, reps, host).  One warm-up call each, then `rounds` rounds in which the variants take turns, one window
    each: what drifts between rounds (clocks, the shared host) reaches all of them alike.  -> {name: sorted ms per call}"""
    for _, fn, _, _ in variants:
        fn()
    out = {name: [] for name, _, _, _ in variants}
    for _ in range(rounds):
        for name, fn, reps, host in variants:
            out[name].append(window(fn, reps, host))
    return {k: sorted(v) for k, v in out.items()}


def traffic(N):
    """bytes the two paths request, from the shapes (tables: floats)"""
    from multiply_amd import hip
    V, J = 6890, 24
    v_template, shapedirs, posedirs, j_reg, lbs_w, verts = 3 * V * 4, 3 * V * 10 * 4, 207 * 3 * V * 4, J * V * 4, V * J * 4, 3 * V * 4
    # mp_smpl_pose per row: shape (v_template, shapedirs -> v_shaped), joints (j_regressor, 24 x v_shaped), verts (posedirs,
    # lbs_weights, v_shaped -> verts)
    loop_row = v_template + shapedirs + verts + j_reg + J * verts + posedirs + lbs_w + verts + verts
    # mp_smpl_pose_batch: per row the chain's v_template, shapedirs and j_regressor and the vertex output; per call posedirs,
    # shapedirs, v_template and lbs_weights once; per row and vertex tile the row's pose feature, transforms and parameters
    tiles = -(-V // 32)
    batch = N * (v_template + shapedirs + j_reg + verts) + posedirs + shapedirs + v_template + lbs_w + N * tiles * (207 + 288 + 14) * 4
    return dict(loop=N * loop_row, loop_posedirs=N * posedirs, batch=batch, batch_posedirs=posedirs, work=N * hip.SMPL_BATCH_ROW_WORK * 4)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--persons", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=int, default=350, help="about how long one timed window of a variant lasts")
    args = ap.parse_args(argv)
    from multiply_amd import hip, pose_metrics
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_scene, make_smpl_tables
    hip.require_device()
    F, P = args.frames, args.persons
    rng = np.random.RandomState(0)
    base = make_scene(P, seed=0, H=16, W=16)["smpl_params"][0]
    gt = np.repeat(base[None], F, 0).astype(np.float32)
    gt[:, :, 4:76] += rng.normal(0, 0.2, (F, P, 72)).astype(np.float32)
    pred = gt.copy()
    pred[:, :, 4:76] += rng.normal(0, 0.02, (F, P, 72)).astype(np.float32)
    pred[:, :, 1:4] += rng.normal(0, 0.01, (F, P, 3)).astype(np.float32)
    tables = make_smpl_tables(0)
    servers = [SMPLServer(gender="male", betas=base[p, 76:], smpl_tables=tables) for p in range(P)]
    sv = servers[0]
    rows = torch.from_numpy(np.concatenate([pred.reshape(-1, 86), gt.reshape(-1, 86)])).cuda()
    N = rows.shape[0]
    f32 = dict(dtype=torch.float32, device="cuda")
    v, t, j = torch.empty(N, 6890, 3, **f32), torch.empty(N, 24, 4, 4, **f32), torch.empty(N, 24, 3, **f32)

    def loop():
        for i in range(N):
            sv.pose_into(rows[i], v[i], t[i], j[i])
    loop()
    out = sv.pose_batch(rows)
    diff = [(out[k] - x).abs().max().item() for k, x in (("verts", v), ("tfs", t), ("joints", j))]
    tr = traffic(N)
    print(f"{torch.cuda.get_device_name(0)}; {F} frames x {P} persons, prediction and ground truth = {N} parameter rows; synthetic tables")
    print(f"loop : {N} x mp_smpl_pose = {4 * N} launches, {tr['loop'] / 1e9:.2f} GB requested, {tr['loop_posedirs'] / 1e9:.2f} GB of it posedirs "
          f"({N} reads of 17.1 MB)")
    print(f"batch: 1 x mp_smpl_pose_batch = 2 launches, {tr['batch'] / 1e9:.2f} GB requested, {tr['batch_posedirs'] / 1e6:.1f} MB of it posedirs "
          f"(one read); work buffer {tr['work'] / 1e6:.2f} MB")
    print(f"max |batch - loop|: verts {diff[0]:.2e}  tfs {diff[1]:.2e}  joints {diff[2]:.2e}")
    k = max(1, args.window_ms // 70)                   # windows of about window_ms for every variant
    variants = [(f"{N} x pose_into (host loop)", loop, k, False),
                ("1 x pose_batch, all outputs", lambda: sv.pose_batch(rows), 50 * k, False),
                ("1 x pose_batch, verts + joints", lambda: sv.pose_batch(rows, want=("verts", "joints")), 50 * k, False),
                ("pose_metrics, whole call (host clock)", lambda: pose_metrics.pose_metrics(pred, gt, servers=servers), 25 * k, True)]
    res = alternated(variants, args.rounds)
    print(f"{args.rounds} rounds, the variants in turn within each; calls per window: " + ", ".join(str(v[2]) for v in variants) + "; ms per call, sorted")
    rows_out = [(name, res[name]) for name, _, _, _ in variants]
    for name, ts in rows_out:
        print(f"{name:40s} " + "  ".join(f"{x:9.3f}" for x in ts) + "  ms")
    mid = args.rounds // 2
    t_loop, t_batch = rows_out[0][1][mid], rows_out[1][1][mid]
    print(f"spread (max - min) / median: loop {(rows_out[0][1][-1] - rows_out[0][1][0]) / t_loop:.2%}, batch {(rows_out[1][1][-1] - rows_out[1][1][0]) / t_batch:.2%}")
    print(f"loop / batch (median rounds): {t_loop / t_batch:.1f} x; the batch moves {tr['batch'] / t_batch / 1e9:.2f} TB/s of what it requests "
          f"(tables come out of the caches), {N * 6890 * 3 * (207 + 10) / t_batch / 1e9:.2f} T multiply-adds / s in the blend shapes")


if __name__ == "__main__":
    main()
