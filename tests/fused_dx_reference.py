"""float64 restatement of mp_tf_sdf_dx (csrc/tfuse.hip k_tf_sdf_dx): the value sweep's share of the adjoint of the input
points of the foreground SDF net, from the adjoints of the pre-activations of layers 0 and 4.

    dIN [P][39] = dZ_0 W_0[:, 0:39] + (1/sqrt 2) dZ_4 W_4[:, 217:256]
    dx  [P][3]  = J_PE(x)^T dIN,   PE(x) = [x, sin(2^k x), cos(2^k x) for k = 0..5]  (embedders.py: 3 columns per block)

Shared by tests/test_fused_pose_grad_cpu.py (which pins it against torch autograd) and tests/test_fused_pose_grad_gpu.py (which
holds the kernel to it)."""
import math

import torch

E_PE, OUT3, MULTIRES = 39, 217, 6


def fused_dx_reference(dZ0, dZ4, W0, W4, x, dx0=None):
    """dZ0, dZ4 [P][256]; W0 [256][>= 39] (Fourier columns first), W4 [256][256] (Fourier columns 217..255); x [P][3];
    dx0 [P][3]: what the kernel accumulates onto (None = zeros).
    -> dx [P][3] (float64) and S [P][3], the sum of the absolute values of every term that enters a component of dx: the
    scale of a rounding-error bound that holds whatever the order of summation."""
    f64 = lambda t: t.detach().double().cpu()
    dZ0, dZ4, W0, W4, x = f64(dZ0), f64(dZ4), f64(W0)[:, :E_PE], f64(W4)[:, OUT3:OUT3 + E_PE], f64(x)
    r2 = 1.0 / math.sqrt(2.0)
    dIN = dZ0 @ W0 + r2 * (dZ4 @ W4)
    sIN = dZ0.abs() @ W0.abs() + r2 * (dZ4.abs() @ W4.abs())
    dx, S = dIN[:, 0:3].clone(), sIN[:, 0:3].clone()
    for k in range(MULTIRES):
        f = float(2 ** k)
        sn, cs = torch.sin(x * f), torch.cos(x * f)
        c_sin, c_cos = 3 + 6 * k, 3 + 6 * k + 3           # columns of sin(f x_a), cos(f x_a), a = 0..2
        dx += f * (cs * dIN[:, c_sin:c_sin + 3] - sn * dIN[:, c_cos:c_cos + 3])
        S += f * (cs.abs() * sIN[:, c_sin:c_sin + 3] + sn.abs() * sIN[:, c_cos:c_cos + 3])
    if dx0 is not None:
        dx += f64(dx0)
        S += f64(dx0).abs()
    return dx, S
