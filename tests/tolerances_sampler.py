"""Limits of tests/test_sampler_kernels_gpu.py (k_sampler_init / k_sampler_bound / k_sampler_resample called directly).

Most of what that file asserts is exact (the merge, the sorts, the picks, flags, counters, untouched rows) and has no limit.
The rest are RESIDUALS: the float64 reference of tests/sampler_reference.py is evaluated at the kernel's own result and the
condition that defines the result must hold to the limits below.  None of them was fitted to a device figure.

INIT_Z_ULPS = 4 (ulps of the ray's far, per depth; NE <= 256, near <= far / 8).  t = linspace(0, 1, NE)[i] is
fl(fl(1 / (NE-1)) * i) below the middle (relative 2 * 2^-24 on t <= 1/2: 2^-24 absolute) and fl(1 - fl(step * k)) above it (2^-24
from the product <= 1/2, 2^-25 from the subtraction): |dt| <= 1.5 * 2^-24, so far * dt <= 1.5 ulp(far) (ulp(far) > far * 2^-24).  The
product fl(far * t) and the sum with near * (1 - t) add half an ulp each, the near term itself less than half: 3 ulp without
jitter.  With jitter, lower and upper are means of two such depths (3 ulp, plus half for the rounded sum), the result is a convex
combination of the two (3.5 ulp) whose final addition rounds once more (0.5 ulp; the difference upper - lower and its product
with t_rand are far / NE in size and round at that scale): 4 ulp.

INIT_BETA_REL = 1e-6 against the float64 formula ON THE DEVICE'S OWN znew.  (Against the reference's depths the figure would
not be one of the beta stage: a depth error e_i of an ulp of far moves sum d_i^2 by 2 sum d_i (e_{i+1} - e_i), which for
independent roundings is 2 sqrt(2 NE) 2^-24 relative, 2.7e-6 at NE = 256 -- the depths' limit, not beta's.)  fl(1 + eps)
is off by 2^-24 relative, which the logarithm near 1.1 amplifies by 1 / ln 1.1 = 10.5: 6.3e-7 relative on log(1 + eps), half of it
after the square root (3.1e-7).  The differences of neighbouring depths are exact or correctly rounded, their squares
correctly rounded, and at most 4 per lane plus 6 levels of the wave sum are added: <= 10 * 2^-24 on the sum, 3e-7 after the root.
logf, the division, the product and sqrtf add about 2^-24 each (halved where they sit under the root): 1.5e-7.  Sum 7.6e-7.

DELTA_E = 16 x max(CPU_SPREAD_E, 6e-6), relative, on the error bound E(beta).
    CPU_SPREAD_E: the largest |E32 - E64| / E64 of the reference's own float32 and float64 evaluations at the float64 root of
    E(beta) = eps, over every ray of the GPU file's line-search cases whose bound crosses eps between beta0 and beta_prev
    (sampler_reference.root_spread; test_sampler_reference_cpu.py reproduces the figure).  6e-6 is what csrc/sampler.hip states
    for its v_exp_f32 exponentials.  16: the bound multiplies up to three such exponentials, the wave scans add in another
    order than a sequential sum, and |d ln E / d ln beta| reaches 8 (0.65 .. 1.9 on these cases).  A dropped term, a wrong
    interval or a shifted scan moves E by percent.

DELTA_CDF = 1e-5 + 8 x max(CPU_SPREAD_CDF, 1e-6), absolute, on the cdf value of a returned depth.
    1e-5: the reference's own rule that bins narrower than 1e-5 in the cdf are not interpolated (ray_sampler.py:183).
    CPU_SPREAD_CDF: the largest |cdf32 - cdf64| of the reference's two evaluations over the SHARP rays of the resample cases
    (sharp: that difference is <= 1e-5; at least 24 of the 37 rays of every case, asserted on the CPU).  The rays that are not
    sharp miss or graze the surface: their pdf is the float32 cancellation noise of exp(x) - 1 over a total of about
    n * 1e-5, which belongs to the algorithm; they get every exact check and no value check.
    To DELTA_CDF the test adds 4 ulp32(z) x the local slope of the float64 cdf: the float32 rounding of the interpolated depth
    itself (with beta = 1e-3 nearly all mass can sit in a bin a millimetre wide).

LATTICE = 1e-2: after J <= 10 halvings the returned beta is beta0 + m w, w = (beta_prev - beta0) / 2^J, m integer in [1, 2^J].  Each
midpoint rounds by half an ulp and later halvings halve what earlier ones left: one ulp of beta in all, 1.2e-7 beta at
most, against w >= 0.1 beta0 / 1024 on the generated states: 1.2e-3 of a step.

DEVICE_RESIDUAL_E / DEVICE_RESIDUAL_CDF: the worst residuals measured on an MI355X over every case of the GPU file -- for E the
largest relative amount by which a condition `E64 <= eps` or `E64 >= eps` was missed before DELTA_E is granted (0: every
condition held outright), for the cdf the largest distance of u to the cdf interval less the slope term.  For the record;
the tests assert against the limits above, never against these."""

INIT_Z_ULPS = 4
INIT_BETA_REL = 1e-6

CPU_SPREAD_E = 5.22e-7
CPU_SPREAD_CDF = 1.18e-6
DELTA_E = 16 * max(CPU_SPREAD_E, 6e-6)
DELTA_CDF = 1e-5 + 8 * max(CPU_SPREAD_CDF, 1e-6)
LATTICE = 1e-2

DEVICE_RESIDUAL_E = 6.93e-7        # (64, 192, 0.001, 'perturbed'), 30 halvings
DEVICE_RESIDUAL_CDF = 9.94e-6      # n = 768, a bin below the 1e-5 rule; 7.8e-6 on the lists up to 320
DEVICE_INIT = (1.88, 1.9e-7)       # znew in ulp of far, beta relative (limits INIT_Z_ULPS, INIT_BETA_REL)
