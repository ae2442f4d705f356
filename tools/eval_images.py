#!/usr/bin/env python
"""Image metrics between a folder of rendered frames and a folder of ground-truth frames (multiply_amd/image_metrics.py:
definitions in its docstring).
    python tools/eval_images.py PRED_DIR GT_DIR [--mask-dir DIR] [--pred-mask-dir DIR --gt-mask-dir DIR] [--as-saved]
The PNGs of the two folders are paired by sorted name; the counts and the sizes must agree.  --mask-dir: one mask PNG per frame
(non-zero = inside) for the masked PSNR / SSIM.  --pred-mask-dir / --gt-mask-dir: one sub-folder per person, each with one mask
PNG per frame (the layout of a scene's mask/<person>/), for the segmentation scores.  Prints one JSON line: the dict of
image_metrics, and under "masks" the dict of mask_metrics."""
import argparse
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def png_paths(folder):
    paths = sorted(glob.glob(os.path.join(folder, "*.png")))
    if not paths:
        raise SystemExit(f"{folder}: no PNG files")
    return paths


def load_frames(folder, n=None, size=None):
    """(N, H, W, 3) uint8 of the folder's PNGs in sorted order; SystemExit unless there are n of them, all of one size (= size)"""
    from multiply_amd.datasets import read_png_rgb
    paths = png_paths(folder)
    if n is not None and len(paths) != n:
        raise SystemExit(f"{folder}: {len(paths)} PNG files, expected {n}")
    frames = [read_png_rgb(p) for p in paths]
    size = frames[0].shape[:2] if size is None else tuple(size)
    for p, f in zip(paths, frames):
        if f.shape[:2] != size:
            raise SystemExit(f"{p}: {f.shape[1]} x {f.shape[0]} pixels, expected {size[1]} x {size[0]}")
    return np.stack(frames)


def load_masks(folder, n, size):
    """(N, H, W) bool: a pixel is inside when any channel of the mask PNG is non-zero"""
    return load_frames(folder, n, size).any(-1)


def load_person_masks(folder, n, size):
    """(N, P, H, W) bool from one sub-folder per person (sorted by name), or from the folder itself for one person"""
    persons = sorted(d for d in glob.glob(os.path.join(folder, "*")) if os.path.isdir(d)) or [folder]
    return np.stack([load_masks(d, n, size) for d in persons], 1)


def jsonable(d):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else jsonable(v) if isinstance(v, dict) else v) for k, v in d.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred_dir")
    ap.add_argument("gt_dir")
    ap.add_argument("--mask-dir", default=None, help="per-frame masks for psnr_masked / ssim_masked")
    ap.add_argument("--pred-mask-dir", default=None, help="predicted person masks (sub-folder per person); needs --gt-mask-dir")
    ap.add_argument("--gt-mask-dir", default=None, help="ground-truth person masks (sub-folder per person)")
    ap.add_argument("--as-saved", action="store_true", help="quantise the prediction as the saved PNGs are (a no-op on PNG input)")
    args = ap.parse_args(argv)
    if (args.pred_mask_dir is None) != (args.gt_mask_dir is None):
        ap.error("--pred-mask-dir and --gt-mask-dir go together")
    from multiply_amd import hip, image_metrics
    hip.require_device()
    pred = load_frames(args.pred_dir)
    n, size = pred.shape[0], pred.shape[1:3]
    gt = load_frames(args.gt_dir, n, size)
    mask = None if args.mask_dir is None else load_masks(args.mask_dir, n, size)
    out = image_metrics.image_metrics(pred, gt, mask=mask, as_saved=args.as_saved)
    if args.pred_mask_dir is not None:
        pm, gm = load_person_masks(args.pred_mask_dir, n, size), load_person_masks(args.gt_mask_dir, n, size)
        if pm.shape != gm.shape:
            raise SystemExit(f"{pm.shape[1]} predicted and {gm.shape[1]} ground-truth persons")
        out["masks"] = image_metrics.mask_metrics(pm, gm)
    out = jsonable(out)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
