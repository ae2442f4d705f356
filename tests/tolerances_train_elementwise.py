"""Limits of tests/test_train_elementwise_gpu.py: per kernel, the largest allowed ratio of |device - float64 reference| to the
per-element bound of tests/train_elementwise_reference.py.

The bound's constants (the same for every kernel; train_elementwise_reference.py derives the bound from them operation by
operation, so there is no per-kernel constant to tune):
    u      = 2^-24    unit roundoff charged per arithmetic operation
    eta    = 2^-150   absolute term per operation (half a denormal step)
    U_F    = 1        ulps allowed per expf / log1pf / sinf / cosf / sqrtf / division
    FLOOR  = 2^-126   added once per element (results that underflow on the device)

CPU_RATIO[kernel]: worst ratio of the HOST's float32 evaluation of the kernel's expression tree to that bound, over
train_elementwise_reference.cpu_ratio_cases() (test_train_elementwise_reference_cpu.py reproduces them within 10 %).
limit(kernel) = max(2, 4 x CPU_RATIO): the device's math library and its fused multiply-adds differ from the host's by a few
ulps per call, not by a factor; a dropped term, a wrong row or a wrong derivative is off by orders of magnitude more.
DEVICE_RATIO[kernel]: the worst ratio measured on an MI355X over every case of the GPU file (for the record; the tests assert
against limit(), never against these)."""

CPU_RATIO = {
    "softplus_fwd": 0.7136, "softplus_bwd": 0.7264, "sigmul": 0.8617, "rev_adj": 0.9132, "dz": 0.8549, "rev_chain": 0.7926,
    "pe": 0.9426, "pe_bwd": 0.5001, "pe_grad_fwd": 0.4070, "pe_grad_bwd": 0.9219, "shade_in_fwd": 0.3246,
    "shade_in_bwd": 0.2613, "sigmoid_fwd": 0.7069, "sigmoid_bwd": 0.5703, "wn_fwd": 0.1042, "wn_bwd": 0.0962,
    "hoist_fwd": 0.01285, "colsum": 0.00157, "bg_comp_fwd": 0.2453, "bg_comp_bwd": 0.5493, "warp_bwd": 0.00385,
}

DEVICE_RATIO = {
    "softplus_fwd": 0.9994, "softplus_bwd": 0.7951, "sigmul": 0.8805, "rev_adj": 0.9531, "dz": 0.8183, "rev_chain": 0.6479,
    "pe": 1.273, "pe_bwd": 0.9985, "pe_grad_fwd": 0.7273, "pe_grad_bwd": 1.27, "shade_in_fwd": 0.3391, "shade_in_bwd": 0.1388,
    "sigmoid_fwd": 0.727, "sigmoid_bwd": 0.6699, "wn_fwd": 0.0706, "wn_bwd": 0.2969, "hoist_fwd": 0.00564, "colsum": 0.01165,
    "bg_comp_fwd": 0.3703, "bg_comp_bwd": 0.6326, "warp_bwd": 0.2465,
}


def limit(kernel):
    return max(2.0, 4.0 * CPU_RATIO[kernel])
