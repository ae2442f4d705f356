#!/usr/bin/env python
"""Are two builds of the library bit-identical in what the MLP kernels compute?   python tools/lib_output_diff.py A.so B.so
Each library is loaded in a fresh child process (MP_LIB_PATH) and evaluates mp_mlp_sdf, mp_mlp_sdf_x2, the shading pair + colour
and mp_background (per-ray and shared depths) on seeded inputs with the "trained" weights of tests/weight_regimes.py
(196 685 points, 4 717 rays: several tiles per workgroup, partial last tiles); the parent compares with torch.equal.
Exit status 1 when any output differs."""
import hashlib, os, subprocess, sys, tempfile
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dump(path):
    sys.path.insert(0, ROOT)
    from multiply_amd import hip
    from tests import weight_regimes as W
    m, _, _ = W.regime_networks("trained", 0)
    m.cuda()
    imp, ren = m.foreground_implicit_network_list[0], m.foreground_rendering_network_list[0]
    n = 3 * 65536 + 77
    lo, hi = W.canonical_bounds()
    x = W.region_points(n, 7001, lo, hi).float().cuda().contiguous()
    cond = W.pose_vector(3000).float().cuda()
    g = torch.Generator().manual_seed(77)
    jinv = (torch.eye(3).reshape(1, 9) + 0.2 * torch.randn(n, 9, generator=g)).cuda().contiguous()
    out = {"sdf": hip.implicit_sdf(imp, x, cond), "sdf_x2": hip.implicit_sdf(imp, x, cond, mode="f16x2")}
    out["shade sdf"], out["shade normal"], out["shade rgb"] = hip.shade_points(imp, ren, x, jinv, cond)
    R = 4717
    d, cam = W.bg_rays(R, 4100)
    d, cam = d.float().cuda(), cam.float().cuda()
    z = (torch.rand(R, 32, generator=g) / 3.0).sort(dim=1, descending=True).values.cuda().contiguous()
    code = m.frame_latent_encoder.weight[W.FRAME].detach().float()
    out["background"] = hip.background(m.bg_implicit_network, m.bg_rendering_network, d, cam, z, code)
    out["background, shared depths"] = hip.background(m.bg_implicit_network, m.bg_rendering_network, d, cam, z[0].contiguous(), code)
    torch.cuda.synchronize()
    torch.save({k: v.cpu() for k, v in out.items()}, path)


if __name__ == "__main__":
    if sys.argv[1] == "--dump":
        dump(sys.argv[2])
        sys.exit(0)
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            lib = os.path.abspath(lib)
            print(f"library {i}: {lib}  sha256 {hashlib.sha256(open(lib, 'rb').read()).hexdigest()[:16]}")
            path = os.path.join(tmp, f"{i}.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--dump", path], env=dict(os.environ, MP_LIB_PATH=lib),
                           check=True, timeout=300)
            res.append(torch.load(path))
    bad = 0
    for k in res[0]:
        eq = torch.equal(res[0][k], res[1][k])
        diff = (res[0][k].double() - res[1][k].double()).abs().max().item()
        print(f"{k:28s} bit-equal: {eq}   max|diff| {diff:.3e}   finite: {bool(torch.isfinite(res[0][k]).all())}")
        bad += not eq
    sys.exit(1 if bad else 0)
