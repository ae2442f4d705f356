#!/usr/bin/env python
"""Pose metrics between a predicted and a ground-truth sequence (multiply_amd/pose_metrics.py: definitions in its docstring).
    python tools/eval_poses.py PRED_DIR GT_DIR [--scale S] [--gender G ...] [--contact-threshold T] [--depth-threshold D]
                                               [--smpl-scale K]
Both folders are in the scene format datasets.py reads: poses.npy (F,P,72), mean_shape.npy (P,10), normalize_trans.npy (F,P,3)
(synthetic.write_sequence writes such folders).  The two sequences must share a frame of reference and the order of their persons.
--scale is unit_scale (multiplies the distances: 100 for metres -> centimetres); --gender one per person or one for all (default:
GT_DIR/gender.npy, else neutral); --contact-threshold builds the contact correspondences from the ground-truth bodies (in the
bodies' own unit) and adds cd / cd_gt; depths for pcdr are the world z.  Prints the dict of pose_metrics as one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_params(root, smpl_scale=1.0):
    """(F, P, 86) float32 = [scale, transl, thetas, betas] of a scene folder"""
    poses = np.load(os.path.join(root, "poses.npy")).astype(np.float32)
    trans = np.load(os.path.join(root, "normalize_trans.npy")).astype(np.float32)
    shape = np.load(os.path.join(root, "mean_shape.npy")).astype(np.float32)
    if poses.ndim != 3 or poses.shape[2] != 72 or trans.shape != poses.shape[:2] + (3,) or shape.shape != (poses.shape[1], 10):
        raise ValueError(f"{root}: expected poses.npy (F,P,72), normalize_trans.npy (F,P,3), mean_shape.npy (P,10), got "
                         f"{poses.shape}, {trans.shape}, {shape.shape}")
    F, P = poses.shape[:2]
    return np.concatenate([np.full((F, P, 1), smpl_scale, np.float32), trans, poses, np.broadcast_to(shape[None], (F, P, 10))], 2)


def genders(arg, gt_dir, P):
    if arg:
        if len(arg) not in (1, P):
            raise ValueError(f"--gender: one value or one per person ({P}), got {len(arg)}")
        return list(arg) * (P if len(arg) == 1 else 1)
    path = os.path.join(gt_dir, "gender.npy")
    return [str(g) for g in np.load(path)][:P] if os.path.exists(path) else ["neutral"] * P


def make_servers(gender_list, betas):
    from multiply_amd.smpl import SMPLServer
    return [SMPLServer(gender=g, betas=b) for g, b in zip(gender_list, betas)]


def jsonable(out):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pred")
    ap.add_argument("gt")
    ap.add_argument("--scale", type=float, default=1.0, help="unit_scale: multiplies the distances")
    ap.add_argument("--gender", nargs="*", default=[], help="body model per person (or one for all)")
    ap.add_argument("--contact-threshold", type=float, default=None, help="build contacts from the ground truth; the bodies' unit")
    ap.add_argument("--depth-threshold", type=float, default=0.15, help="pcdr: in the scaled unit")
    ap.add_argument("--smpl-scale", type=float, default=1.0, help="the scale entry of the 86 parameters of both sequences")
    args = ap.parse_args(argv)
    from multiply_amd import hip, pose_metrics
    hip.require_device()
    pred, gt = load_params(args.pred, args.smpl_scale), load_params(args.gt, args.smpl_scale)
    if pred.shape != gt.shape:
        raise ValueError(f"the sequences differ in (F, P): {pred.shape[:2]} and {gt.shape[:2]}")
    servers = make_servers(genders(args.gender, args.gt, gt.shape[1]), gt[0, :, 76:])
    contacts = None
    if args.contact_threshold is not None:              # pose the ground truth once: for the contacts and for the scores
        verts, joints = pose_metrics.pose_sequence(servers, gt)
        contacts = pose_metrics.contacts_from_bodies(verts, servers[0].faces, args.contact_threshold)
        gt = {"verts": verts, "joints": joints}
    out = pose_metrics.pose_metrics(pred, gt, servers=servers, unit_scale=args.scale, contacts=contacts,
                                    depth_threshold=args.depth_threshold)
    print(json.dumps(jsonable(out)))
    return out


if __name__ == "__main__":
    main()
