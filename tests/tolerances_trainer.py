"""Bounds of tests/test_trainer_gpu.py.  mp_adam_multi is compared with the float64 step of tests/trainer_reference.py from
identical fp32 state:
    |p' - p64'|  <=  half an ulp of p64'  +  C_P * 2^-24 * |p64' - p|        per element
    |m' - m64'|  <=  C_MV * 2^-24 * |m64'|   (the same for v')               per element
C_P and C_MV are TWICE what torch's own CPU fp32 Adam (torch.optim.Adam(foreach=False)) needs against the same float64 step on
the same table (trainer_reference.make_state(0), make_grads(1)): measured there, never on the kernel.
tests/test_trainer_cpu.py measures the two values again and checks that they are not above the ones recorded here.  The moments'
constant is as large as it is because exp_avg' = m + 0.1 (g - m) cancels where g is near -9 m: the difference g - m is rounded
at its own, larger, magnitude."""
# Below FLT_MIN fp32 has no relative precision: its values are spaced 2^-149 apart whatever their size.  Real gradients reach that
# range (exp_avg_sq' = 0.001 g^2 is subnormal for |g| < 3.4e-18), so the moments' bound carries the format's own spacing as an
# absolute floor, C_MV * 2^-149; on the tables of tests 1 - 3 (all values far above FLT_MIN) it changes nothing.
FLT_MIN = 2.0 ** -126
SUBNORMAL_SPACING = 2.0 ** -149
TORCH_CPU_C_P = 4.570        # measured: 4.5697
TORCH_CPU_C_MV = 16.863      # measured: 16.8625
C_P = 2 * TORCH_CPU_C_P
C_MV = 2 * TORCH_CPU_C_MV
CHAIN_STEPS = 20
