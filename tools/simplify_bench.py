#!/usr/bin/env python
"""Times the mesh simplification (multiply_amd/simplify.py) on the validation-size extraction of tests/bench_mesh.py: person 0's
canonical level set of the seeded, untrained test model at res_up (default 4: a 513^3 lattice, about 1.3 M faces), at cell sizes
of 2, 4 and 8 lattice spacings and for one face-count target.

    stages    device time between events recorded at the end of every stage of simplify_mesh, median over --reps runs after a
              warm-up; the stages named `torch:` are torch's sorts, unique and prefix sums, the others the kernels of
              csrc/simplify.hip with the host read-backs that follow them (the counts that size the next allocation)
    quality   metrics.mesh_metrics(simplified, original): Chamfer distance (metres and lattice spacings), normal consistency
    reference the float64 statement of the algorithm (tests/mesh_simplify_reference.py, numpy, one CPU thread), once, at the middle
              cell size, and whether the device's faces equal its

Prints a table and one JSON line.  What this is not: a trained body (the level set of the initialised network is smoother than
a trained one, so fewer faces meet at sharp features), and a single mesh (Trainer.test simplifies one mesh per person and frame,
each paying the host read-backs that this run amortises over nothing either)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from multiply_amd import hip, metrics                            # noqa: E402
from multiply_amd.mesh import generate_mesh                       # noqa: E402
from multiply_amd.simplify import simplify_mesh                   # noqa: E402
from tests import mesh_simplify_reference as R                    # noqa: E402
from tests.test_render_gpu import build                           # noqa: E402


def staged(verts, faces, reps, **kw):
    """({stage: median ms}, total median ms, the result)"""
    simplify_mesh(verts, faces, **kw)                             # warm-up: allocator, sort workspaces
    runs = []
    for _ in range(reps):
        ev = []
        torch.cuda.synchronize()
        out = simplify_mesh(verts, faces, stages=ev, **kw)
        torch.cuda.synchronize()
        runs.append([(name, a.elapsed_time(b)) for (_, a), (name, b) in zip(ev[:-1], ev[1:])])
    names = [n for n, _ in runs[0]]
    med = {n: float(np.median([r[i][1] for r in runs])) for i, n in enumerate(names)}
    return med, float(np.median([sum(t for _, t in r) for r in runs])), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res-up", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacings", type=float, nargs="*", default=[2.0, 4.0, 8.0], help="cell sizes in lattice spacings")
    ap.add_argument("--target", type=int, default=50_000)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    model, _, _ = build(H=9, W=9)
    imp = model.foreground_implicit_network_list[0]
    cond = torch.zeros(69, device="cuda")
    vc = model.smpl_server_list[0].verts_c[0]
    with torch.no_grad():
        m = generate_mesh(lambda x: hip.implicit_sdf(imp, x.contiguous(), cond), vc, 0.0, 32, a.res_up)
    verts, faces = m.vertices_t.contiguous(), m.faces_t.contiguous()
    ext = (vc.max(0).values - vc.min(0).values).max().item()
    spacing = 1.1 * ext / m.resolution
    info = dict(res_up=a.res_up, lattice=m.resolution + 1, verts=int(verts.shape[0]), faces=int(faces.shape[0]), spacing=spacing,
                reps=a.reps, runs=[])
    print(f"mesh: lattice {m.resolution + 1}^3, {verts.shape[0]} vertices, {faces.shape[0]} faces, lattice spacing {spacing * 1e3:.3f} mm; "
          f"{a.reps} runs each after a warm-up, medians")
    jobs = [(f"cell = {s:g} spacings", dict(cell=float(np.float32(s * spacing)))) for s in a.spacings]
    jobs.append((f"target_faces = {a.target}", dict(target_faces=a.target)))
    for name, kw in jobs:
        med, total, (v2, f2, inf) = staged(verts, faces, a.reps, **kw)
        q = metrics.mesh_metrics((v2, f2), (verts, faces), n_samples=a.samples)
        torch_ms = sum(t for n, t in med.items() if n.startswith("torch:"))
        rec = dict(name=name, cell=inf["cell"], passes=inf["passes"], faces_after=int(f2.shape[0]), verts_after=int(v2.shape[0]),
                   n_duplicate=inf["n_duplicate"], n_unreferenced=inf["n_unreferenced"], total_ms=total, torch_ms=torch_ms,
                   stages_ms=med, chamfer=q["chamfer"], chamfer_spacings=q["chamfer"] / spacing, hausdorff=q["hausdorff"],
                   normal_consistency=q["normal_consistency"])
        info["runs"].append(rec)
        print(f"\n{name}: cell {inf['cell'] * 1e3:.3f} mm, {inf['passes']} count passes -> {f2.shape[0]} faces, {v2.shape[0]} vertices "
              f"({inf['n_duplicate']} duplicates, {inf['n_unreferenced']} unreferenced cells)")
        for n, t in med.items():
            print(f"    {n:48s} {t:9.3f} ms")
        print(f"    {'total':48s} {total:9.3f} ms   of which torch's sorts and prefix sums {torch_ms:.3f} ms ({100 * torch_ms / total:.0f} %)")
        print(f"    against the original ({a.samples} samples a side): Chamfer {q['chamfer'] * 1e3:.4f} mm = {q['chamfer'] / spacing:.3f} spacings, "
              f"Hausdorff {q['hausdorff'] * 1e3:.3f} mm, normal consistency {q['normal_consistency']:.5f}")
    if not a.no_reference and len(a.spacings):
        s = a.spacings[len(a.spacings) // 2]
        h = float(np.float32(s * spacing))
        vn, fn = verts.cpu().numpy(), faces.cpu().numpy()
        t0 = time.perf_counter()
        ref = R.simplify(vn, fn, h)
        t_ref = time.perf_counter() - t0
        v2, f2, _ = simplify_mesh(verts, faces, cell=h)
        same = bool(np.array_equal(f2.cpu().numpy(), ref["faces"]))
        err = float(np.abs(v2.cpu().numpy().astype(np.float64) - ref["verts64"]).max()) if same else float("nan")
        info["reference"] = dict(cell=h, seconds=t_ref, faces_equal=same, max_position_error=err)
        print(f"\nfloat64 reference (numpy, one thread) at cell = {s:g} spacings: {t_ref:.1f} s; faces equal the device's: {same}; "
              f"positions differ by at most {err:.3e} m")
    print(json.dumps(info))


if __name__ == "__main__":
    main()
