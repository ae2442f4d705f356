#!/usr/bin/env python
"""Times the device work of multiply_amd.scene_build on a sequence (default 300 frames x 2 persons at 1080 x 1920, synthetic SMPL
tables, seeded poses): the batched path

    SMPLServer.pose_batch + mp_verts_bounds (both forms) + mp_raster_mask_batch + mp_mask_dilate + mp_mask_stats (raw and dilated)

against the loop the code before scene_build allows

    SMPLServer.pose_batch + torch.amin / amax + the norm in torch, Renderer.rasterize per mesh (zbuf >= 0),
    torch.nn.functional.max_pool2d with the same window and anchor per frame, and the counts / boxes with torch reductions.

Both run in ONE process, alternating, `--reps` times each after a warm-up of every shape, timed with device events; before any
timing the masks of the two paths are compared byte for byte.  Prints a table of the stages and one JSON line.  `--only batched`
runs that path alone (for a kernel trace)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--persons", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--dilate", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("both", "batched"), default="both")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from multiply_amd import scene_build as SB
    from multiply_amd.render import Renderer
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_smpl_tables

    dev = torch.device("cuda")
    F, P, (H, W), k = a.frames, a.persons, a.size, a.dilate
    server = SMPLServer(smpl_tables=make_smpl_tables(0))
    faces = torch.from_numpy(np.ascontiguousarray(server.faces)).to(dev)
    rs = np.random.RandomState(a.seed)
    fx = 1.3 * H
    K = np.array([[fx, 0, W / 2.0], [0, fx, H / 2.0], [0, 0, 1.0]])
    prm = np.zeros((F, P, 86), np.float32)
    prm[..., 0] = 1.0
    t = np.linspace(0, 1, F)[:, None]
    for p in range(P):
        prm[:, p, 1:4] = np.array([(p - (P - 1) / 2.0) * 0.9, 0.15, 3.6 + 0.5 * p]) + t * rs.normal(0, 0.3, 3) + rs.normal(0, 0.01, (F, 3))
        prm[:, p, 4:7] = np.array([np.pi, 0, 0]) + rs.normal(0, 0.1, 3) + t * rs.normal(0, 0.2, 3)
        prm[:, p, 7:76] = rs.normal(0, 0.2, 69) + t * rs.normal(0, 0.2, 69)
        prm[:, p, 76:] = rs.normal(0, 0.5, 10)
    prm = torch.from_numpy(prm).to(dev)
    cam16 = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, fx, fx, W / 2.0, H / 2.0]         # the fits are in camera space already
    shift = torch.zeros(F, 3, device=dev)
    ren = Renderer(img_size=[H, W], cam_intrinsic=K)
    ay = k // 2

    def pose():
        return torch.stack([server.pose_batch(prm[:, p].contiguous(), absolute=True, want=("verts",))["verts"] for p in range(P)], 1)

    def batched(verts, keep):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        flat = verts.reshape(F, -1, 3)
        bounds, norm = SB.verts_bounds(flat), SB.verts_bounds(flat, shift)
        ev[1].record()
        raw = SB.raster_mask_batch(verts.reshape(F * P, -1, 3), faces, cam16, H, W, out=keep.get("raw"))
        ev[2].record()
        dil = SB.mask_dilate(raw, k)
        ev[3].record()
        st = (SB.mask_stats(raw), SB.mask_stats(dil))
        ev[4].record()
        return ev, dict(raw=raw, dil=dil, stats=st, bounds=bounds, norm=norm)

    def loop(verts, keep):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        flat = verts.reshape(F, -1, 3)
        bounds = torch.cat([torch.amin(flat, 1), torch.amax(flat, 1)], 1)
        norm = (flat + shift[:, None]).norm(dim=-1).amax(1)
        ev[1].record()
        raw = keep.get("raw")
        raw = torch.empty(F * P, H, W, dtype=torch.uint8, device=dev) if raw is None else raw
        v = verts.reshape(F * P, -1, 3)
        for i in range(F * P):
            raw[i] = (ren.rasterize(v[i], faces).zbuf[0, :, :, 0] >= 0).to(torch.uint8) * 255
        ev[2].record()
        dil = torch.empty_like(raw)
        for f in range(F):                                   # a frame at a time: the float copy of the whole sequence is 4 x the masks
            x = torch.nn.functional.pad(raw[f * P:(f + 1) * P].float()[:, None], (ay, k - 1 - ay, ay, k - 1 - ay))
            dil[f * P:(f + 1) * P] = torch.nn.functional.max_pool2d(x, k, stride=1)[:, 0].to(torch.uint8)
        ev[3].record()
        st = []
        for m in (raw, dil):
            nz = m > 0
            rows, cols = nz.any(2), nz.any(1)
            st.append((nz.sum((1, 2)), rows.float().argmax(1), H - 1 - rows.flip(1).float().argmax(1), cols.float().argmax(1),
                       W - 1 - cols.flip(1).float().argmax(1)))
        ev[4].record()
        return ev, dict(raw=raw, dil=dil, stats=st, bounds=bounds, norm=norm)

    def times(ev):
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]

    verts = pose()
    torch.cuda.synchronize()
    # warm-up of every shape + the byte-for-byte comparison
    _, b = batched(verts, {})
    torch.cuda.synchronize()
    info = {"frames": F, "persons": P, "size": [H, W], "dilate": k, "reps": a.reps,
            "mask_bytes": int(b["raw"].numel()), "covered_fraction_raw": float((b["raw"] > 0).float().mean()),
            "covered_fraction_dilated": float((b["dil"] > 0).float().mean())}
    keep_b, keep_l = {"raw": b["raw"]}, {}
    if a.only == "both":
        _, l = loop(verts, {})
        torch.cuda.synchronize()
        info["masks_equal"] = bool(torch.equal(b["raw"], l["raw"]))
        info["mask_pixels_differing"] = int((b["raw"] != l["raw"]).sum())
        info["dilated_equal"] = bool(torch.equal(b["dil"], l["dil"]))
        info["bounds_equal"] = bool(torch.equal(b["bounds"], l["bounds"]))
        sb = b["stats"][1]
        info["stats_equal"] = bool(all(torch.equal(sb[:, i], l["stats"][1][i].long()) for i in range(5)))
        if not (info["masks_equal"] and info["dilated_equal"] and info["bounds_equal"] and info["stats_equal"]):
            print(json.dumps(info))
            raise SystemExit("the two paths disagree: nothing is timed")
        keep_l = {"raw": l["raw"]}
        del l
    del b
    stages = ("bounds", "raster", "dilate", "stats")
    tb, tl, tp = [], [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        verts = pose()
        e1.record()
        ev, _r = batched(verts, keep_b)
        tb.append(times(ev))
        tp.append(e0.elapsed_time(e1))
        del _r
        if a.only == "both":
            ev, _r = loop(verts, keep_l)
            tl.append(times(ev))
            del _r
    tb, tl = np.array(tb), np.array(tl)
    info["pose_batch_ms"] = [float(np.median(tp)), float(np.min(tp)), float(np.max(tp))]
    print(f"{F} frames x {P} persons at {H} x {W}, dilate {k}: masks {info['mask_bytes'] / 1e9:.3f} GB, covered {info['covered_fraction_raw']:.3f} "
          f"raw / {info['covered_fraction_dilated']:.3f} dilated; pose_batch {info['pose_batch_ms'][0]:.3f} ms")
    print(f"{'stage':8s} {'batched ms: median  min  max':36s} {'loop ms: median  min  max':36s} ratio")
    for i, s in enumerate(stages + ("total",)):
        col = lambda t: t.sum(1) if s == "total" else t[:, i]
        mb = [float(np.median(col(tb))), float(col(tb).min()), float(col(tb).max())]
        info["batched_" + s + "_ms"] = mb
        line = f"{s:8s} {mb[0]:12.3f} {mb[1]:10.3f} {mb[2]:10.3f}   "
        if a.only == "both":
            ml = [float(np.median(col(tl))), float(col(tl).min()), float(col(tl).max())]
            info["loop_" + s + "_ms"] = ml
            line += f"{ml[0]:12.3f} {ml[1]:10.3f} {ml[2]:10.3f}   {ml[0] / mb[0]:8.2f}"
        print(line)
    print(json.dumps(info))


if __name__ == "__main__":
    main()
