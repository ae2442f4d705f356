#!/usr/bin/env python
"""Times the overlay images of a sequence (default 300 frames x 2 SMPL bodies at 512 x 512, synthetic SMPL tables, seeded poses):

    batched   overlay.vertex_normals + overlay.vertex_colors('normal') + overlay.render_overlays, one call per
              --images-per-call chunk, both bodies z-tested into their frame
    loop      the only way before overlay.py: Renderer.render_mesh_recon(mode='n') per mesh (normals in torch, the soft
              rasteriser with its host read of the tile-list length) and a torch blend of the RGBA result over the frame,
              one body after the other

Both run in ONE process, alternating, `--reps` rounds each after a warm-up, timed on the host around a device synchronisation
(the loop's cost IS its host round trips).  The two paths draw by different rules (nearest face / 10-face depth softmax), so the
pictures are compared by their covered sets only.  Prints a table and one JSON line; `--only batched` runs that path alone."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--persons", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512), metavar=("H", "W"))
    ap.add_argument("--images-per-call", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("both", "batched"), default="both")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from multiply_amd import overlay as OV
    from multiply_amd.render import Renderer
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_smpl_tables

    dev = torch.device("cuda")
    F, P, (H, W) = a.frames, a.persons, a.size
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
    verts = torch.stack([server.pose_batch(prm[:, p].contiguous(), absolute=True, want=("verts",))["verts"] for p in range(P)], 1)
    verts = verts.reshape(F * P, -1, 3).contiguous()                                        # (frame, person) order
    cam16 = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, fx, fx, W / 2.0, H / 2.0]           # the fits are in camera space
    frames = torch.from_numpy(rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)).to(dev)
    image_of = [i // P for i in range(F * P)]
    adj = tuple(torch.from_numpy(x).to(dev) for x in OV.vertex_adjacency(faces, verts.shape[1]))
    ren = Renderer(img_size=[H, W], cam_intrinsic=K)

    def batched():
        nrm = OV.vertex_normals(verts, faces, adj)
        return OV.render_overlays((verts, faces, OV.vertex_colors(nrm, "normal")), image_of, cam16, H, W, frames=frames,
                                  images_per_call=a.images_per_call)

    def loop():
        out = frames.clone()
        for i in range(F * P):
            rgba = ren.render_mesh_recon(verts[i], faces, mode="n")[0]                      # (H, W, 4) over white, A = coverage
            al = rgba[..., 3:]
            f = i // P
            out[f] = (255 * rgba[..., :3] * al + out[f].float() * (1 - al)).clamp(0, 255).to(torch.uint8)
        return out

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    _, b = timed(batched)                                                                    # warm-up of every shape
    info = {"frames": F, "persons": P, "size": [H, W], "faces_per_mesh": int(faces.shape[0]), "images_per_call": a.images_per_call,
            "reps": a.reps, "changed_fraction_batched": float((b != frames).any(-1).float().mean())}
    if a.only == "both":
        _, l = timed(loop)
        cb, cl = (b != frames).any(-1), (l != frames).any(-1)
        info["changed_fraction_loop"] = float(cl.float().mean())
        info["covered_sets_differ_fraction"] = float((cb != cl).float().mean())
        del l
    del b
    tb, tl = [], []
    for _ in range(a.reps):
        tb.append(timed(batched)[0])
        if a.only == "both":
            tl.append(timed(loop)[0])
    stat = lambda x: [float(np.median(x)), float(np.min(x)), float(np.max(x))]
    info["batched_ms"] = stat(tb)
    print(f"{F} frames x {P} bodies at {H} x {W} ({info['faces_per_mesh']} faces each), {a.reps} alternating rounds")
    print(f"{'path':8s} {'ms: median':>12s} {'min':>10s} {'max':>10s}")
    print(f"{'batched':8s} {info['batched_ms'][0]:12.3f} {info['batched_ms'][1]:10.3f} {info['batched_ms'][2]:10.3f}")
    if a.only == "both":
        info["loop_ms"] = stat(tl)
        info["loop_over_batched"] = info["loop_ms"][0] / info["batched_ms"][0]
        print(f"{'loop':8s} {info['loop_ms'][0]:12.3f} {info['loop_ms'][1]:10.3f} {info['loop_ms'][2]:10.3f}   x {info['loop_over_batched']:.1f}")
    print(json.dumps(info))


if __name__ == "__main__":
    main()
