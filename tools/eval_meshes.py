#!/usr/bin/env python
"""Metrics between a reconstructed mesh and a ground-truth one (multiply_amd/metrics.py: definitions in its docstring).
    python tools/eval_meshes.py PRED.ply GT.ply [--samples N] [--thresholds T ...] [--iou-res R] [--scale S] [--seed K]
                                [--align {rigid,similarity}] [--align-samples N] [--align-iters K] [--save-aligned PATH]
    python tools/eval_meshes.py PRED_DIR GT_DIR [...] [--align-shared]
Prints the dict of mesh_metrics as one JSON line.  --align registers the prediction onto the ground truth first
(multiply_amd/registration.py); --save-aligned writes the transformed prediction as a PLY (a folder, when the arguments are
folders).  With two folders the PLY files are matched by name and the line is {"frames": {name: dict}, "mean": {key: mean},
"unmatched": {...}}; --align-shared then fits ONE transform to all frames (registration.register_sequence) instead of one each."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def match_folders(pred_dir, gt_dir):
    """([(name, pred path, gt path)] sorted by name, {"pred": [...], "gt": [...]} names without a partner): the .ply files of the
    two folders matched by file name"""
    ply = lambda d: {f for f in os.listdir(d) if f.lower().endswith(".ply") and os.path.isfile(os.path.join(d, f))}
    a, b = ply(pred_dir), ply(gt_dir)
    pairs = [(f, os.path.join(pred_dir, f), os.path.join(gt_dir, f)) for f in sorted(a & b)]
    return pairs, {"pred": sorted(a - b), "gt": sorted(b - a)}


def mean_of(dicts):
    """the means of the per-frame dicts: floats by key, lists of floats element by element; other entries are left out"""
    out = {}
    for k in dicts[0] if dicts else ():
        vals = [d[k] for d in dicts if k in d]
        if all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals):
            out[k] = sum(vals) / len(vals)
        elif all(isinstance(v, list) and all(isinstance(x, (int, float)) for x in v) for v in vals) and len({len(v) for v in vals}) == 1:
            out[k] = [sum(col) / len(col) for col in zip(*vals)]
    return out


def write_ply(path, verts, faces):
    """a binary little-endian triangle PLY (what metrics.load_ply reads)"""
    import numpy as np
    v, f = np.ascontiguousarray(verts, "<f4"), np.ascontiguousarray(faces, "<i4")
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rec["n"], rec["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\nproperty float x\nproperty float y\n"
                  f"property float z\nelement face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred")
    ap.add_argument("gt")
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="in the scaled unit, at most 8")
    ap.add_argument("--iou-res", type=int, default=None, help="lattice points per axis of volume_iou (closed meshes only)")
    ap.add_argument("--scale", type=float, default=1.0, help="unit_scale: multiplies the distances")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--align", choices=("rigid", "similarity"), default=None, help="register the prediction onto the ground truth first")
    ap.add_argument("--align-samples", type=int, default=20000, help="samples per mesh of the registration")
    ap.add_argument("--align-iters", type=int, default=30, help="at most this many ICP iterations")
    ap.add_argument("--align-shared", action="store_true", help="folders: one transform for all frames (register_sequence)")
    ap.add_argument("--save-aligned", default=None, metavar="PATH", help="write the aligned prediction (folders: a folder)")
    args = ap.parse_args(argv)
    folders = os.path.isdir(args.pred) and os.path.isdir(args.gt)
    if (args.align_shared or args.save_aligned) and not args.align:
        ap.error("--align-shared and --save-aligned need --align")
    if args.align_shared and not folders:
        ap.error("--align-shared needs two folders")
    from multiply_amd import hip, metrics
    hip.require_device()
    kw = dict(n_samples=args.samples, thresholds=args.thresholds, seed=args.seed, unit_scale=args.scale, iou_resolution=args.iou_res)
    opts = dict(n_samples=args.align_samples, max_iters=args.align_iters)

    def one(pred, gt, align, save):
        if align is None:           # the call of before the registration existed, argument for argument
            return metrics.mesh_metrics(pred, gt, **kw)
        out = metrics.mesh_metrics(pred, gt, align=align, align_options=opts if isinstance(align, str) else None, **kw)
        if save:
            from multiply_amd import registration as reg
            v, f = metrics.as_mesh(pred)
            T = reg.Similarity.from_matrix(out["align"]["matrix"])
            write_ply(save, reg.transform_vertices(v, T).cpu().numpy(), f.cpu().numpy())
        return out

    if not folders:
        out = one(args.pred, args.gt, args.align, args.save_aligned)
        print(json.dumps(out))
        return out
    pairs, unmatched = match_folders(args.pred, args.gt)
    if not pairs:
        ap.error("the two folders share no .ply file name")
    if args.save_aligned:
        os.makedirs(args.save_aligned, exist_ok=True)
    align, shared = args.align, None
    if args.align_shared:
        from multiply_amd import registration as reg
        align, info = reg.register_sequence([p for _, p, _ in pairs], [g for _, _, g in pairs], kind=args.align, seed=args.seed, **opts)
        shared = dict(kind=args.align, scale=align.scale, matrix=align.matrix.tolist(), rms=info["rms"],
                      iterations=info["iterations"], converged=info["converged"])
    frames = {name: one(p, g, align, os.path.join(args.save_aligned, name) if args.save_aligned else None) for name, p, g in pairs}
    out = dict(frames=frames, mean=mean_of(list(frames.values())), unmatched=unmatched)
    if shared is not None:
        out["align"] = shared
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
