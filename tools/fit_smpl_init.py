"""Fit a foreground ImplicitNet to a body surface and write the smpl_init file Multiply loads (multiply_amd/smpl_init.py).

    python tools/fit_smpl_init.py --out outputs/smpl_init_male_256.pth                       # the synthetic body (closed_body_mesh)
    python tools/fit_smpl_init.py --out outputs/smpl_init_male_256.pth --gender male         # real SMPL tables, where installed
    python tools/fit_smpl_init.py --out scan_init.pth --mesh scan.ply                        # any closed triangle mesh (binary PLY)

Then set `smpl_init: true` and `smpl_init_path: <file>` in the model config.  One fit per process; from a job script run it under
its own `timeout -k 10 <seconds>`.  Prints the fit record and the held-out error (mean / max |sdf - exact distance| on 4 096
surface and 4 096 box points)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_ply(path):
    """binary little-endian PLY with float x y z vertices and uchar-counted int triangles (what ExtractedMesh.export writes)"""
    with open(path, "rb") as fh:
        nv = nf = None
        while True:
            line = fh.readline().decode("ascii", "replace").strip()
            if line.startswith("format") and "binary_little_endian" not in line:
                raise ValueError("only binary_little_endian PLY files are read")
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            if line.startswith("element face"):
                nf = int(line.split()[-1])
            if line == "end_header":
                break
        v = np.frombuffer(fh.read(12 * nv), dtype="<f4").reshape(nv, 3)
        rec = np.frombuffer(fh.read(13 * nf), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        if not (rec["n"] == 3).all():
            raise ValueError("only triangle faces are read")
    return v.astype(np.float32), rec["i"].astype(np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--gender", default=None, help="fit to the canonical surface of the real SMPL tables of this gender")
    ap.add_argument("--mesh", default=None, help="fit to this closed triangle mesh (binary PLY)")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-every", type=int, default=0)
    a = ap.parse_args()
    import torch
    from multiply_amd import smpl_init as S
    from multiply_amd.config import load_config
    from multiply_amd.networks import ImplicitNet
    from multiply_amd.smpl import SMPLServer
    cfg = S.FitConfig(seed=a.seed)
    if a.steps is not None:
        cfg.steps = a.steps
    if a.mesh:
        v, f = read_ply(a.mesh)
    elif a.gender:
        server = SMPLServer(gender=a.gender, betas=np.zeros(10, dtype=np.float32))
        v, f = server.verts_c[0], torch.as_tensor(np.asarray(server.smpl.faces).astype(np.int64))
    else:
        from multiply_amd.synthetic import closed_body_mesh, make_smpl_tables
        server = SMPLServer(gender="male", betas=np.zeros(10, dtype=np.float32), smpl_tables=make_smpl_tables(0))
        v, f = closed_body_mesh(server)
    torch.manual_seed(0)
    net = ImplicitNet(load_config().implicit_network).to("cuda")
    before = S.heldout_error(net, v, f)
    t0 = time.perf_counter()
    rec = S.fit_implicit_net(net, v, f, cfg=cfg, log_every=a.log_every)
    total = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    S.save_smpl_init(net, a.out)
    print(rec)
    for step, terms in rec.terms:
        print(f"  step {step}: " + ", ".join(f"{k} {x:.4e}" for k, x in terms.items()))
    print(f"total fit time {total:.2f} s")
    print("held-out error before: " + ", ".join(f"{k} {x:.4e}" for k, x in before.items()))
    print("held-out error after:  " + ", ".join(f"{k} {x:.4e}" for k, x in S.heldout_error(net, v, f).items()))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
