#!/usr/bin/env python
"""Times the image-metric kernels (csrc/image_metrics.hip) on a rendered-sequence-sized input and, as the yardstick, the same SSIM
written with torch.nn.functional.conv2d in float64 on the device (the 11 x 11 window in one convolution, and as two 1-D passes).
    python tools/image_metrics_bench.py [--frames 75] [--size 512] [--reps 20]
Device events around `reps` back-to-back calls after a warm-up, three rounds each (the spread is printed); the frames are mostly
flat background with a textured patch, as a render is.  The text it prints is what profiles/image_metrics.txt holds."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, rounds=3, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return sorted(out)


def taps64(dev):
    k = torch.arange(11, dtype=torch.float64, device=dev) - 5
    g = torch.exp(-k * k / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_conv2d(a, b, separable):
    """per-frame mean SSIM (N,) with float64 convolutions: the textbook E[x^2] - mu^2 form, which float64 can afford"""
    N, H, W, C = a.shape
    x = a.permute(0, 3, 1, 2).reshape(N * C, 1, H, W).double()
    y = b.permute(0, 3, 1, 2).reshape(N * C, 1, H, W).double()
    g = taps64(a.device)

    def filt(t):
        if separable:
            return F.conv2d(F.conv2d(t, g.reshape(1, 1, 1, 11)), g.reshape(1, 1, 11, 1))
        return F.conv2d(t, torch.outer(g, g).reshape(1, 1, 11, 11))
    mx, my = filt(x), filt(y)
    vx, vy, cxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    s = (2 * mx * my + 1e-4) * (2 * cxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    return s.reshape(N, -1).mean(1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=75)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    from multiply_amd import hip
    hip.require_device()
    N, S, C = args.frames, args.size, 3
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.full((N, S, S, C), 0.9, device="cuda") + 1e-3 * torch.rand(N, S, S, C, generator=g, device="cuda")
    q = S // 4
    a[:, q:3 * q, q:3 * q] = torch.rand(N, 2 * q, 2 * q, C, generator=g, device="cuda")
    b = (a + 0.05 * (torch.rand(N, S, S, C, generator=g, device="cuda") - 0.5)).clamp(0, 1)
    mask = torch.zeros(N, S, S, dtype=torch.bool, device="cuda")
    mask[:, q:3 * q, q:3 * q] = True
    in_bytes = 2 * a.numel() * 4
    n_map = N * (S - 10) * (S - 10) * C
    T = hip.SSIM_TILE
    tiles = (-(-(S - 10) // T)) ** 2
    staged = N * tiles * C * 2 * (T + 10) ** 2 * 4
    print(f"{torch.cuda.get_device_name(0)}; {N} frames {S} x {S} x {C} float32; {args.reps} calls per round, 3 rounds (ms per call, sorted)")
    print(f"one pass over both images = {in_bytes / 1e6:.1f} MB; the algorithmic minimum for PSNR and SSIM is two reads of each image "
          f"(one per kernel) = {2 * in_bytes / 1e6:.1f} MB; SSIM map values {n_map / 1e6:.2f} M, ~{n_map * 110 / 1e9:.2f} G fp64 multiply-adds")
    print(f"mp_image_ssim requests {staged / 1e6:.1f} MB = {staged / in_bytes:.2f} passes (tile + halo = ({T}+10)^2 / {T}^2; the channels of a "
          f"pixel share cache lines, so a tile's three channel passes hit the cache); mp_image_sqerr reads 1.00 pass: "
          f"{1 + staged / in_bytes:.2f} against the minimum of 2")
    rows = []
    rows.append(("mp_image_ssim (sums only)", timed(lambda: hip.image_ssim(a, b), args.reps)))
    rows.append(("mp_image_ssim + mask", timed(lambda: hip.image_ssim(a, b, mask), args.reps)))
    rows.append(("mp_image_ssim + map (fp32 out)", timed(lambda: hip.image_ssim(a, b, want_map=True), args.reps)))
    rows.append(("mp_image_sqerr", timed(lambda: hip.image_sqerr(a, b), args.reps)))
    rows.append(("mp_image_sqerr + mask", timed(lambda: hip.image_sqerr(a, b, mask), args.reps)))
    ours = (hip.image_ssim(a, b)[0][:, 0] / hip.image_ssim(a, b)[0][:, 1]).cpu()
    for name, sep in (("conv2d float64, two 1-D passes", True), ("conv2d float64, one 11 x 11 window", False)):
        try:
            rows.append((name, timed(lambda: ssim_conv2d(a, b, sep), max(1, args.reps // 10), warmup=1)))
            d = (ssim_conv2d(a, b, sep).cpu() - ours).abs().max().item()
            print(f"{name}: max |mean SSIM - mp_image_ssim's| over the frames = {d:.2e}")
        except Exception as e:                     # a float64 convolution the library does not have: say so, time the rest
            print(f"{name}: not measured ({type(e).__name__}: {str(e)[:200]})")
        torch.cuda.empty_cache()
    for name, t in rows:
        print(f"{name:38s} " + "  ".join(f"{v:9.3f}" for v in t))
    t_ssim, t_sq = rows[0][1][1], rows[3][1][1]
    print(f"mp_image_ssim: {n_map * 110 / t_ssim / 1e9:.2f} T fp64 multiply-adds / s (median round); "
          f"mp_image_sqerr: {in_bytes / t_sq / 1e9:.2f} TB/s of the {in_bytes / 1e6:.0f} MB it must read")
    conv = [t for n, t in rows if n.startswith("conv2d")]
    if conv:
        print("conv2d / kernel (median rounds): " + ", ".join(f"{t[1] / t_ssim:.1f} x" for t in conv))


if __name__ == "__main__":
    main()
