#!/usr/bin/env python
"""Train a scene folder end to end (multiply_amd/trainer.py; what code/train.py does with Lightning and hydra).
    python tools/train.py --scene DIR [--conf YAML] --out DIR --epochs N [--resume] [--rays 512] [--seed 42] [--synthetic-smpl]
                          [--sam-checkpoint FILE] [--deterministic]
--scene: a folder in the layout datasets.Hi4DDataset reads (tools/build_scene.py writes one).  --conf: a model config in the layout
of multiply_amd/confs/model.yaml (default: that file); the schedule keys of trainer.SCHEDULE_DEFAULTS go there too.  --out: the run
folder (stage files, rendering/, checkpoints/).  --resume: continue from the newest OUT/checkpoints/epoch=*.ckpt, or from last.ckpt
when that file is more recent.
--synthetic-smpl: the seeded synthetic body tables instead of the licensed SMPL model (scenes of synthetic.write_sequence).
--sam-checkpoint: build segment_anything's predictor from this file for the mask stage; without it the stage is skipped.
--deterministic: the deterministic training mode (the config key `deterministic`): with --seed, the same run gives the same bits.
Prints one JSON line per epoch: the epoch's mean loss terms, steps, skipped NaN steps, learning rate, seconds and ms per step."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--conf", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, required=True)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--rays", type=int, default=512)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--synthetic-smpl", action="store_true")
    ap.add_argument("--sam-checkpoint", default=None)
    ap.add_argument("--deterministic", action="store_true")
    args = ap.parse_args(argv)
    import torch
    from multiply_amd import trainer as T
    from multiply_amd.config import load_config
    predictor = None
    if args.sam_checkpoint:
        from segment_anything import SamPredictor, sam_model_registry
        predictor = SamPredictor(sam_model_registry["vit_h"](checkpoint=args.sam_checkpoint).to("cuda"))
    tables = None
    if args.synthetic_smpl:
        from multiply_amd.synthetic import make_smpl_tables
        tables = make_smpl_tables(0)
    lines = []
    opt = load_config(args.conf)
    if args.deterministic:
        opt["deterministic"] = True
    tr = T.build_trainer(args.scene, args.out, opt=opt, dataset_opt=dict(num_sample=args.rays),
                         sam_predictor=predictor, smpl_tables=tables, seed=args.seed, log=lines.append)
    if args.resume:
        # the newest epoch=*.ckpt as code/train.py:44 takes it, or last.ckpt when that is the more recent file (this tool writes one
        # when it ends)
        found = [p for p in (T.newest_checkpoint(os.path.join(tr.out_dir, "checkpoints")),
                             os.path.join(tr.out_dir, "checkpoints", "last.ckpt")) if p and os.path.exists(p)]
        if not found:
            raise SystemExit(f"--resume: no checkpoint under {tr.out_dir}/checkpoints")
        tr.load_checkpoint(max(found, key=os.path.getmtime))
    for epoch in range(tr.epoch, args.epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log = tr.fit(epoch + 1)[-1]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        log.update(seconds=dt, ms_per_step=1e3 * dt / max(log["steps"], 1))
        for line in lines[:-1]:                      # the stages' notes (skipped stage, failed mesh refresh)
            print(line, file=sys.stderr)
        del lines[:]
        print(json.dumps(log), flush=True)
    with T._working_dir(tr.out_dir):
        tr.save_checkpoint(os.path.join("checkpoints", "last.ckpt"))


if __name__ == "__main__":
    main()
