#!/usr/bin/env python
"""The test run of a trained scene (multiply_amd/trainer.py Trainer.test; code/test.py + test_step_each_person).
    python tools/test.py --scene DIR --ckpt FILE --out DIR [--conf YAML] [--frames 0 1 ...] [--synthetic-smpl]
Writes OUT/test_mesh/<p>/, test_rendering/<id>/, test_fg_rendering/<id>/, test_normal/<id>/, test_mask/<id>/ and
test_instance_mask/<p>/ (id -1 = all persons): the folders tools/eval_images.py and tools/eval_meshes.py take.  --ckpt: a
checkpoint of tools/train.py, or any torch.save dict with a 'state_dict' in the same key layout.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--conf", default=None)
    ap.add_argument("--frames", type=int, nargs="*", default=None)
    ap.add_argument("--synthetic-smpl", action="store_true")
    args = ap.parse_args(argv)
    import torch
    from multiply_amd import trainer as T
    from multiply_amd.config import load_config
    tables = None
    if args.synthetic_smpl:
        from multiply_amd.synthetic import make_smpl_tables
        tables = make_smpl_tables(0)
    tr = T.build_trainer(args.scene, args.out, opt=load_config(args.conf), smpl_tables=tables, log=lambda *a: None)
    ck = tr.load_checkpoint(os.path.abspath(args.ckpt))
    t0 = time.perf_counter()
    tr.test(frames=args.frames)
    torch.cuda.synchronize()
    n = len(tr.testset) if args.frames is None else len(args.frames)
    print(json.dumps({"frames": n, "epoch": ck.get("epoch"), "out": tr.out_dir, "seconds": time.perf_counter() - t0}))


if __name__ == "__main__":
    main()
