"""Seeded test images of the image-metric tests (tests/test_image_metrics_*.py): the contents a renderer produces and the ones
that break an fp32-moment SSIM."""
import numpy as np

CONTENTS = ("noise", "8bit", "flat", "ramp", "const")


def pair(content, shape, seed=0):
    """(a, b) float32 arrays of `shape` = (N, H, W, C); the frames of a pair differ from one another"""
    N, H, W, C = shape
    g = np.random.default_rng([seed, N, H, W, C, CONTENTS.index(content)])
    if content == "noise":                   # uniform noise
        a, b = g.random(shape), g.random(shape)
    elif content == "8bit":                  # 8-bit-quantised noise
        a, b = np.floor(g.random(shape) * 256).clip(0, 255) / 255.0, np.floor(g.random(shape) * 256).clip(0, 255) / 255.0
    elif content == "flat":                  # 0.9 + 1e-3 noise: flat background with a little texture
        a, b = 0.9 + 1e-3 * g.random(shape), 0.9 + 1e-3 * g.random(shape)
    elif content == "ramp":                  # a horizontal ramp (per frame and channel a little steeper) against its 0.9 x + 0.05 copy
        x = np.linspace(0.0, 1.0, W)[None, None, :, None]
        gain = 1.0 - 0.05 * np.arange(N)[:, None, None, None] - 0.02 * np.arange(C)[None, None, None, :]
        a = np.broadcast_to(x * gain, shape).astype(np.float32)
        return np.ascontiguousarray(a), np.ascontiguousarray(a * np.float32(0.9) + np.float32(0.05))
    elif content == "const":                 # two constant images (another pair of constants per frame)
        n = np.arange(N)[:, None, None, None]
        a, b = np.broadcast_to(0.3 + 0.1 * n, shape), np.broadcast_to(0.8 - 0.1 * n, shape)
    else:
        raise KeyError(content)
    return np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


def random_mask(shape, seed=0, p=0.4):
    """(N, H, W) bool, neither empty nor full in any frame"""
    N, H, W, _ = shape
    m = np.random.default_rng([seed, N, H, W]).random((N, H, W)) < p
    m[:, 0, 0], m[:, H - 1, W - 1] = True, False
    return m
