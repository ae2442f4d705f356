#!/usr/bin/env python
"""Metrics between a reconstructed mesh and a ground-truth one (multiply_amd/metrics.py: definitions in its docstring).
    python tools/eval_meshes.py PRED.ply GT.ply [--samples N] [--thresholds T ...] [--iou-res R] [--scale S] [--seed K]
Prints the dict of mesh_metrics as one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred")
    ap.add_argument("gt")
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="in the scaled unit, at most 8")
    ap.add_argument("--iou-res", type=int, default=None, help="lattice points per axis of volume_iou (closed meshes only)")
    ap.add_argument("--scale", type=float, default=1.0, help="unit_scale: multiplies the distances")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    from multiply_amd import hip, metrics
    hip.require_device()
    out = metrics.mesh_metrics(args.pred, args.gt, n_samples=args.samples, thresholds=args.thresholds, seed=args.seed,
                               unit_scale=args.scale, iou_resolution=args.iou_res)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
