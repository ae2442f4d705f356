#!/usr/bin/env python
"""Refines the SMPL fits of a scene to its 2D keypoints (multiply_amd.keypoint_fit.refine_sequence: the `refine` mode of the
reference's preprocessing, preprocessing/preprocessing_multiple_trace.py:360-527).

The scene folder holds
  init_smpl.npz            pose (F, P, 72), trans (F, P, 3), shape (F, P, 10): the per-frame initial values, in camera space
  keypoints/*.npy          one file per frame in sorted order, (P, K, 3) = (u, v, confidence): OpenPose's 25 body keypoints
                           (--format coco25) or ViTPose's 17 (--format coco17)
  intrinsics.npy           (3, 3)
  J_regressor_extra.npy    optional (9, 6890): the reference's extra joint regressor, needed by coco17's hips
  extrinsic.npy            optional (3, 4) / (4, 4) world-to-camera, identity without it
  frames/*.png             optional, one per frame in sorted order: needed by --overlays
and receives refined_smpl.npz (pose, trans, shape, terms (F, P, 3), flags (F, P)).  --overlays DIR writes the QC images
DIR/init/<p>/%04d.png and DIR/refined/<p>/%04d.png: the body before / after the fit in normal colours over the frame, the detected
keypoints above the confidence threshold in red, the model's projected keypoints in green (multiply_amd.overlay).  Prints one JSON
line of summary."""
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
    ap.add_argument("scene")
    ap.add_argument("--format", choices=("coco25", "coco17"), default="coco25")
    ap.add_argument("--gender", nargs="+", default=["neutral"], help="one for all persons, or one per person")
    ap.add_argument("--smpl-dir", default=None, help="folder of SMPL_<GENDER>.pkl (default: $MULTIPLY_SMPL_DIR)")
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--conf-threshold", type=float, default=0.6)
    ap.add_argument("--interpolate-frames", type=int, nargs="*", default=[])
    ap.add_argument("--tracking", type=int, nargs="*", default=[], help="frame person frame person ...")
    ap.add_argument("--out", default=None)
    ap.add_argument("--overlays", default=None, metavar="DIR", help="write DIR/init/<p>/ and DIR/refined/<p>/ (needs SCENE/frames/*.png)")
    a = ap.parse_args()
    from multiply_amd import keypoint_fit as KF
    from multiply_amd.smpl import SMPLServer, load_smpl_tables

    init = dict(np.load(os.path.join(a.scene, "init_smpl.npz")))
    files = sorted(glob.glob(os.path.join(a.scene, "keypoints", "*.npy")))
    if not files:
        raise SystemExit(f"no keypoints/*.npy under {a.scene}")
    kps = np.stack([np.load(f) for f in files]).astype(np.float32)
    F, P = init["pose"].shape[:2]
    if kps.shape[0] != F:
        raise SystemExit(f"{len(files)} keypoint files against {F} frames of initial values")
    if len(a.tracking) % 2:
        raise SystemExit("--tracking takes (frame, person) pairs")
    frames = sorted(glob.glob(os.path.join(a.scene, "frames", "*.png")))
    if a.overlays is not None and len(frames) != F:
        raise SystemExit(f"--overlays draws over the frames: {len(frames)} frames/*.png against {F} frames of initial values")
    extra = os.path.join(a.scene, "J_regressor_extra.npy")
    extra = np.load(extra) if os.path.exists(extra) else None
    kmap = getattr(KF.KeypointMap, a.format)(extra)
    cam = {"intrinsics": np.load(os.path.join(a.scene, "intrinsics.npy"))}
    if os.path.exists(os.path.join(a.scene, "extrinsic.npy")):
        cam["extrinsic"] = np.load(os.path.join(a.scene, "extrinsic.npy"))
    genders = a.gender if len(a.gender) > 1 else a.gender * P
    if len(genders) != P:
        raise SystemExit(f"--gender: expected 1 or {P} values, got {len(genders)}")
    servers = {g: SMPLServer(smpl_tables=load_smpl_tables(g, a.smpl_dir)) for g in sorted(set(genders))}
    t0 = time.perf_counter()
    out = KF.refine_sequence([servers[g] for g in genders], {k: torch.from_numpy(np.asarray(init[k], np.float32)) for k in ("pose", "trans", "shape")},
                             torch.from_numpy(kps), cam, kmap, iters=a.iters, lr=a.lr, conf_threshold=a.conf_threshold,
                             interpolate_frames=a.interpolate_frames, tracking=list(zip(a.tracking[::2], a.tracking[1::2])))
    res = {k: out[k].cpu().numpy() for k in ("pose", "trans", "shape", "terms", "flags")}      # (the first host read: synchronises)
    dt = time.perf_counter() - t0
    path = a.out or os.path.join(a.scene, "refined_smpl.npz")
    np.savez(path, **res)
    if a.overlays is not None:
        from multiply_amd import overlay as OV
        for name, fit in (("init", init), ("refined", res)):
            OV.write_fit_overlays(os.path.join(a.overlays, name), [servers[g] for g in genders], fit, kps, kmap, cam, frames,
                                  conf_threshold=a.conf_threshold)
    print(json.dumps({"tool": "refine_smpl", "scene": os.path.abspath(a.scene), "frames": F, "persons": P, "format": a.format,
                      "iters": a.iters, "keypoints": kmap.K, "support_vertices": kmap.S, "notes": kmap.notes,
                      "mean_total_loss": float(np.nanmean(res["terms"][..., 2])), "mean_l2d": float(np.nanmean(res["terms"][..., 0])),
                      "flagged_person_frames": int(res["flags"].sum()), "seconds": dt, "out": os.path.abspath(path),
                      **({"overlays": os.path.abspath(a.overlays)} if a.overlays is not None else {})}))


if __name__ == "__main__":
    main()
