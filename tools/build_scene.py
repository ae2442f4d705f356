#!/usr/bin/env python
"""Builds the scene folder multiply_amd.datasets trains on from refined SMPL fits (multiply_amd.scene_build.build_scene: the `final`
mode of the reference's preprocessing, preprocessing/preprocessing_multiple_trace.py:529-599, and its normalize_cameras_trace.py).

RAW holds
  refined_smpl.npz     pose (F, P, 72), trans (F, P, 3), shape (F, P, 10) in camera space: what tools/refine_smpl.py writes
  intrinsics.npy       (3, 3)
  extrinsic.npy        optional (3, 4) / (4, 4) world-to-camera, identity without it
  frames/*.png         optional, one per frame in sorted order; without them no image/ is written and --img-size is needed
OUT receives image/, mask/<person>/, poses.npy, mean_shape.npy, normalize_trans.npy, gender.npy, cameras.npz, max_human_sphere.npy
and cameras_normalize.npz; with --overlays (needs frames) also the QC images overlay/<person>/ (the body in normal colours over the
frame) and overlay/all/ (all persons tinted, z-tested against each other).  Prints one JSON line of summary."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("raw")
    ap.add_argument("out")
    ap.add_argument("--normalize", choices=("per-frame", "first-frame"), default="per-frame")
    ap.add_argument("--dilate", type=int, default=20)
    ap.add_argument("--scale-factor", type=int, default=1)
    ap.add_argument("--gender", nargs="+", default=["neutral"], help="one for all persons, or one per person")
    ap.add_argument("--smpl-dir", default=None, help="folder of SMPL_<GENDER>.pkl (default: $MULTIPLY_SMPL_DIR)")
    ap.add_argument("--img-size", type=int, nargs=2, default=None, metavar=("H", "W"), help="only without RAW/frames")
    ap.add_argument("--overlays", action="store_true", help="write OUT/overlay/<person>/ and OUT/overlay/all/ (needs RAW/frames)")
    a = ap.parse_args()
    from multiply_amd import scene_build as SB
    from multiply_amd.smpl import SMPLServer, load_smpl_tables

    refined = dict(np.load(os.path.join(a.raw, "refined_smpl.npz")))
    F, P = refined["pose"].shape[:2]
    frames = sorted(glob.glob(os.path.join(a.raw, "frames", "*.png"))) or None
    if frames is not None:
        if len(frames) != F:
            raise SystemExit(f"{len(frames)} frames against {F} frames of fits")
        from PIL import Image
        with Image.open(frames[0]) as im:
            img_size = (im.size[1], im.size[0])
    elif a.img_size is None:
        raise SystemExit(f"no frames/*.png under {a.raw}: give --img-size H W")
    else:
        img_size = tuple(a.img_size)
    if a.overlays and frames is None:
        raise SystemExit(f"--overlays draws over the frames: no frames/*.png under {a.raw}")
    ext = os.path.join(a.raw, "extrinsic.npy")
    ext = np.load(ext) if os.path.exists(ext) else None
    genders = a.gender if len(a.gender) > 1 else a.gender * P
    if len(genders) != P:
        raise SystemExit(f"--gender: expected 1 or {P} values, got {len(genders)}")
    servers = {g: SMPLServer(smpl_tables=load_smpl_tables(g, a.smpl_dir)) for g in sorted(set(genders))}
    t0 = time.perf_counter()
    sc = SB.build_scene([servers[g] for g in genders], refined, np.load(os.path.join(a.raw, "intrinsics.npy")), img_size,
                        out_dir=a.out, frames=frames, genders=genders, normalize=a.normalize.replace("-", "_"), dilate=a.dilate,
                        scale_factor=a.scale_factor, extrinsic=ext, overlays=a.overlays)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    H, W = sc["img_size"]
    frac = sc["mask_stats"]["dilated"]["count"] / float(H * W)                       # (F, P)
    print(json.dumps({"tool": "build_scene", "raw": os.path.abspath(a.raw), "frames": F, "persons": P, "image_size": [H, W],
                      "normalize": a.normalize, "dilate": a.dilate, "scale_factor": a.scale_factor,
                      "max_human_sphere": sc["max_human_sphere"], "scale": 1.0 / float(sc["cameras_normalize"]["scale_mat_0"][0, 0]),
                      "covered_fraction_min": [float(x) for x in frac.min(0)], "covered_fraction_mean": [float(x) for x in frac.mean(0)],
                      "empty_mask_person_frames": int((sc["mask_stats"]["raw"]["count"] == 0).sum()), "seconds": dt,
                      "out": os.path.abspath(a.out), **({"overlays": os.path.join(os.path.abspath(a.out), "overlay")} if a.overlays else {})}))


if __name__ == "__main__":
    main()
