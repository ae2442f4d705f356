#!/usr/bin/env python
"""Brute-force mesh signed distance (mp_mesh_signed_distance) against the face index (mp_mesh_index_signed_distance): query, and the
index build on its own.    python tools/mesh_index_bench.py [--out profiles/mesh_index.txt] [--reps 30]
HIP-event timing of single launches on an otherwise idle device, median (min) of `reps` launches after 5 warm-up launches; the
build is timed as a whole (keys, torch.sort, gather, boxes).  Shapes:
  (a) the fit's: 8 192 volume points of smpl_init's default step against synthetic.closed_body_mesh (a 129^3 MISE mesh);
  (b) one person's training flags: the canonical samples of a 512-ray training step against the model's initial face list
      (13 776 faces), against a 129^3 MISE mesh of the body and against the person's own refreshed canonical mesh;
  (c) squashed spheres of 8 * 4^k and 20 * 4^k faces, 8 192 points in their box: where the index starts to win;
  (d) a single query of 5 120 points with the index built for it (interpenetration_loss).
The last column says what 'auto' picks for the mesh (hip.mesh_index_wanted: closed surface, hip.MESH_INDEX_MIN_FACES faces).
Also: boxes tested / faces evaluated per point (the kernel's optional counters), and bit-equality of the two results.
    python tools/mesh_index_bench.py --closest [--big] [--out profiles/mesh_closest.txt]
measures the closest-face query instead (mp_mesh_closest against mp_mesh_index_closest): 100 000 surface samples of a shifted
copy of closed_body_mesh against that mesh (--big: also against its res_up=4 extraction), with and without the Hilbert ordering
of the query points (its two sorts included), and the signed query of the same index on the same points for comparison."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--closest", action="store_true")
ap.add_argument("--big", action="store_true")
args = ap.parse_args()
sys.argv = sys.argv[:1]
import bench  # noqa: E402
from multiply_amd import hip, mesh, smpl_init  # noqa: E402
from multiply_amd.synthetic import closed_body_mesh  # noqa: E402

lines = []
AUTO_ROWS = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=args.reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ts.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(ts), min(ts)


def sphere(k, base):
    """an octahedron (base 8) / icosahedron (base 20) subdivided k times, squashed and offset: (F,3,3)"""
    t = (1 + 5 ** 0.5) / 2
    if base == 8:
        v = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
        f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    else:
        v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
             [-t, 0, -1], [-t, 0, 1]]
        f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
             [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    fv = torch.tensor(v, dtype=torch.float64)[torch.tensor(f)]
    fv = fv / fv.norm(dim=-1, keepdim=True)
    for _ in range(k):
        a, b, c = fv[:, 0], fv[:, 1], fv[:, 2]
        ab, bc, ca = ((x + y) / (x + y).norm(dim=-1, keepdim=True) for x, y in ((a, b), (b, c), (c, a)))
        fv = torch.cat([torch.stack(q, 1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    return (0.5 * fv * torch.tensor([1.0, 1.4, 0.7]) + torch.tensor([0.03, -0.02, 0.05])).float().cuda().contiguous()


def compare(tag, pts, fv, faces=True):
    """one row: brute / index query / build in us, visits, equality, and what 'auto' picks for this mesh (faces: its vertex ids,
    or True for a surface known to be closed); returns (brute, query, build) medians"""
    pts, fv = pts.detach().float().contiguous(), fv.detach().reshape(-1, 9).float().contiguous()
    n, F = pts.shape[0], fv.shape[0]
    sd_b, sd_i = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    tb = timed(lambda: hip.mesh_signed_distance(pts, fv, out=sd_b))
    tbuild = timed(lambda: hip.MeshIndex(fv), reps=max(5, args.reps // 3))
    index = hip.MeshIndex(fv)
    tq = timed(lambda: index.signed_distance(pts, out=sd_i))
    visits = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    index.signed_distance(pts, out=sd_i, visits=visits)
    torch.cuda.synchronize()
    vm = visits.float().mean(0).tolist()
    # a wave walks until its slowest lane is done: the mean over waves of the per-wave maximum is what the hardware executes
    pad = (-n) % 64
    wmax = torch.cat([visits[:, 1].float(), torch.zeros(pad, device="cuda")]).reshape(-1, 64).max(1).values.mean().item()
    eq = torch.equal(sd_b.view(torch.int32), sd_i.view(torch.int32))
    auto = "index" if hip.mesh_index_wanted("auto", F, faces) else "brute"
    AUTO_ROWS.append((tag, auto, tb[0], tq[0], tbuild[0]))
    say(f"  {tag:44s} {n:6d} x {F:6d}  brute {tb[0]:9.1f} ({tb[1]:9.1f})  index {tq[0]:8.1f} ({tq[1]:8.1f})  build {tbuild[0]:7.1f}  "
        f"x{tb[0] / tq[0]:6.1f}   boxes/pt {vm[0]:6.1f} faces/pt {vm[1]:6.1f} (per wave max {wmax:6.1f})  bit-equal {eq}  auto: {auto}")
    return tb[0], tq[0], tbuild[0]


def wave_max(visits, n):
    pad = (-n) % 64
    return torch.cat([visits[:, 1].float(), torch.zeros(pad, device="cuda")]).reshape(-1, 64).max(1).values.mean().item()


def closest_rows(tag, pts, fv, brute_reps):
    """brute force / index with and without sorted points / the signed query, for one mesh; median (min .. max) of the launches"""
    pts, fv = pts.detach().float().contiguous(), fv.detach().reshape(-1, 9).float().contiguous()
    n, F = pts.shape[0], fv.shape[0]

    def spread(fn, reps):
        for _ in range(min(5, reps)):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            ts.append(1e3 * e0.elapsed_time(e1))
        return statistics.median(ts), min(ts), max(ts)
    fmt = lambda t: f"{t[0]:10.1f} ({t[1]:10.1f} .. {t[2]:10.1f})"
    say(f"  {tag}: {n} points x {F} faces")
    index = hip.MeshIndex(fv)
    tbuild = spread(lambda: hip.MeshIndex(fv), max(5, args.reps // 3))
    say(f"    index build                          {fmt(tbuild)}")
    want = None
    if brute_reps:
        tb = spread(lambda: hip.mesh_closest(pts, fv), brute_reps)
        want = hip.mesh_closest(pts, fv)
        say(f"    brute force (d2, face, q)            {fmt(tb)}   [{brute_reps} launches]")
    rows = {}
    for sort_points in (False, True):
        t = spread(lambda: index.closest(pts, sort_points=sort_points), args.reps)
        visits = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
        got = index.closest(pts, visits=visits, sort_points=sort_points)
        torch.cuda.synchronize()
        vm = visits.float().mean(0).tolist()
        # the per-wave maximum is over the lanes as LAUNCHED: in the sorted order when the points are sorted
        lanes = visits
        if sort_points:
            keys = torch.empty(n, dtype=torch.int32, device="cuda")
            hip.lib().mp_mesh_index_point_keys(pts, n, index.buf, keys, hip.stream())
            lanes = visits[torch.sort(keys).indices]
        eq = "n/a" if want is None else all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got))
        rows[sort_points] = t[0]
        say(f"    index, points {'in Hilbert order' if sort_points else 'as given        '}      {fmt(t)}   boxes/pt {vm[0]:6.1f} faces/pt {vm[1]:6.1f} "
            f"(per wave max {wave_max(lanes, n):6.1f})  bit-equal to brute {eq}" + (f"  x{tb[0] / t[0]:7.1f}" if brute_reps else ""))
    if brute_reps == 0:                                           # equality on a subset brute force can afford
        sub = pts[:2048].contiguous()
        eq = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(hip.mesh_closest(sub, fv), index.closest(sub)))
        say(f"    (brute force not timed at this size; bit-equal on the first 2 048 points: {eq})")
    sd = torch.empty(n, device="cuda")
    ts = spread(lambda: index.signed_distance(pts, out=sd), args.reps)
    visits = torch.zeros(n, 2, dtype=torch.int32, device="cuda")
    index.signed_distance(pts, out=sd, visits=visits)
    torch.cuda.synchronize()
    vm = visits.float().mean(0).tolist()
    say(f"    signed query (same index, as given)  {fmt(ts)}   boxes/pt {vm[0]:6.1f} faces/pt {vm[1]:6.1f} (per wave max {wave_max(visits, n):6.1f})")
    return rows


def closest_section(bv, bf, server):
    from multiply_amd import metrics
    say(f"Closest face, brute force vs face index.  {torch.cuda.get_device_name(0)}, one device, one session; library {hip.lib_source_sha16()}")
    say(f"HIP events around single calls, median (min .. max) of {args.reps} after 5 warm-up calls, microseconds.  'Hilbert order' "
        f"includes the key kernel, torch's sort and the un-permutation.  hip.MESH_CLOSEST_SORT_POINTS = {hip.MESH_CLOSEST_SORT_POINTS}")
    say()
    gen = torch.Generator(device="cuda").manual_seed(0)
    shifted = (bv + torch.tensor([0.01, -0.008, 0.006], device=bv.device), bf)
    pts = metrics.surface_samples(shifted, 100_000, gen)[0]
    res = {"body": closest_rows("samples of a shifted copy / closed_body_mesh", pts, bv[bf], brute_reps=max(3, args.reps // 5))}
    if args.big:
        say()
        v4, f4 = closed_body_mesh(server, res_up=4)
        res["big"] = closest_rows("the same samples / closed_body_mesh at res_up=4", pts, v4[f4], brute_reps=0)
    say()
    for k, r in res.items():
        say(f"{k}: Hilbert-ordered points {'faster' if r[True] < r[False] else 'slower'} than as given: {r[True]:.1f} vs {r[False]:.1f} us")


torch.cuda.set_device(0)
hip.require_device()
try:
    smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
except (OSError, subprocess.SubprocessError):
    smi = ""
clk = [l.strip() for l in smi.splitlines() if "sclk" in l][:1]
say(f"Mesh signed distance, brute force vs face index.  {torch.cuda.get_device_name(0)}, one device, otherwise idle; "
    f"sclk at start: {clk[0] if clk else 'n/a'}; library {hip.lib_source_sha16()}")
say(f"HIP events around single launches, median (min) of {args.reps} after 5 warm-up launches, microseconds.  x = brute / index query.")
say()

model, inp, tables, sc = bench.build_model(128, seed=0)
gin = bench.to_dev(inp)
server = model.smpl_server_list[0]
bv, bf = closed_body_mesh(server)
body = bv[bf].contiguous()
if args.closest:
    lines.clear()
    closest_section(bv, bf, server)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
say("(a) the fit's step (smpl_init default: 8 192 volume points) against closed_body_mesh; recorded before: 12 994 us")
cfg = smpl_init.FitConfig()
target = smpl_init.MeshTarget(bv, bf, "cuda", mesh_index_mode="brute")
gen = torch.Generator(device="cuda").manual_seed(0)
pts = smpl_init.fit_step_points(target, cfg, smpl_init.fit_box(cfg, target.verts, "cuda"), smpl_init.make_draws(cfg, gen, "cuda"))[0]
compare("fit volume points / body mesh", pts[cfg.n_surface:], body, bf)
say()

say("(b) one person's canonical samples of a 512-ray training step (current_epoch 101)")
model.train()
g = torch.Generator().manual_seed(0)
sel = torch.randperm(gin["uv"].shape[1], generator=g)[:512].cuda()
tin = dict(gin)
tin["uv"] = gin["uv"][:, sel].contiguous()
tin.update(current_epoch=101, index_outside=torch.zeros(512, dtype=torch.bool, device="cuda"), smpl_pose_last=gin["smpl_pose"] + 0.01)
model(tin)
fg = model._last_train.fg[0]
X = fg["X"][:fg["npts"]].clone()
say(f"  person 0: {fg['Rp']} rays x {fg['npts'] // max(fg['Rp'], 1)} samples")
compare("samples / initial face list (not a surface)", X, model.mesh_face_vertices_list[0], model.mesh_f_cano_list[0])
compare("samples / body mesh (129^3 MISE)", X, body, bf)
model.eval()
own = mesh.canonical_mesh(model, 0)
compare("samples / person's canonical mesh (129^3 MISE)", X, own["vertices"][own["faces"]], own["faces"])
say()

say("(c) squashed spheres, 8 192 uniform points in 1.2 x their box")
rows = []
for k, base in [(1, 8), (1, 20), (2, 8), (2, 20), (3, 8), (3, 20), (4, 8), (4, 20), (5, 8), (5, 20), (6, 8), (6, 20)]:
    fv = sphere(k, base)
    lo, hi = fv.reshape(-1, 3).min(0).values, fv.reshape(-1, 3).max(0).values
    g = torch.Generator(device="cuda").manual_seed(k)
    p = (torch.rand(8192, 3, generator=g, device="cuda") - 0.5) * 1.2 * (hi - lo) + (lo + hi) / 2
    rows.append((fv.shape[0],) + compare(f"sphere {base} x 4^{k}", p, fv))
say()
say("(d) one query of interpenetration_loss's size, 5 120 points, index built for it: brute vs build + query")
for k, base in [(3, 20), (4, 8), (4, 20), (5, 8)]:
    fv = sphere(k, base)
    lo, hi = fv.reshape(-1, 3).min(0).values, fv.reshape(-1, 3).max(0).values
    g = torch.Generator(device="cuda").manual_seed(k)
    p = (torch.rand(5120, 3, generator=g, device="cuda") - 0.5) * 1.2 * (hi - lo) + (lo + hi) / 2
    fvf = fv.reshape(-1, 9)
    sd = torch.empty(5120, device="cuda")
    tb = timed(lambda: hip.mesh_signed_distance(p, fvf, out=sd))
    t1 = timed(lambda: hip.MeshIndex(fvf).signed_distance(p, out=sd))
    say(f"  sphere {base} x 4^{k}  {5120:6d} x {fvf.shape[0]:6d}  brute {tb[0]:9.1f}  build + query {t1[0]:9.1f}  x{tb[0] / t1[0]:6.1f}")
    AUTO_ROWS.append((f"single query, {fvf.shape[0]} faces", "index" if hip.mesh_index_wanted("auto", fvf.shape[0], True) else "brute", tb[0], t1[0], 0.0))
say()
win = [F for F, tb, tq, tbd in rows if tq < tb]
once = [F for F, tb, tq, tbd in rows if tq + tbd < tb]
say(f"index query faster than brute force from F = {min(win) if win else 'never'}; query + one build faster from F = {min(once) if once else 'never'}"
    f" (hip.MESH_INDEX_MIN_FACES = {hip.MESH_INDEX_MIN_FACES})")
lost = [(tag, tb, tq + tbd) for tag, auto, tb, tq, tbd in AUTO_ROWS if auto == "index" and tq + tbd >= tb]
say(f"shapes where 'auto' picks the index: {sum(a == 'index' for _, a, *_ in AUTO_ROWS)} of {len(AUTO_ROWS)}; of those, slower than brute force "
    f"(query + one whole build): {lost if lost else 'none'}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
