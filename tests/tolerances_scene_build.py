"""Bounds of tests/test_scene_build_cpu.py and tests/test_scene_build_gpu.py.

Byte, integer and min / max comparisons are exact and have no entry here.

HOST_*: float64 arithmetic on the host against the float64 restatement (tests/scene_build_reference.py).  Both sides round at
2.2e-16 relative; the quantities are metres of order 1 - 10 after a few dozen operations (a chain of up to ten 4 x 4 products in the
body, one matrix -> rotation vector inversion, one 3 x 3 solve), and pixels of order 1e3.  The bounds leave four to five decimal
orders above that and stay eight orders below the smallest defect of interest (a millimetre, a hundredth of a pixel); the tests
print what they measure (largest seen: 4.4e-16 in the root rotation, 7.1e-15 m in estimate_translation, 2.2e-15 in the splines).

Device bounds: 4 x the largest value measured on the MI355X against the float64 restatement over the cases of the test, the
convention of tolerances_keypoint_fit.py and tolerances_penetration.py; the measured value stands next to each bound.  A failure a
little above a bound after a compiler change means RE-MEASURE (the tests print every figure) and record the new value here and in
DESIGN.md section 6k; a failure far above it is a defect."""
MARGIN = 4.0

HOST_METRES = 1e-9
HOST_PIXELS = 1e-6
# The identity  Rt v' = Rc v + tc  is exact for a body whose root rotates by exp(r).  SMPL's batch_rodrigues (lib/smpl/lbs.py:276-307)
# reads a rotation vector r as the angle t' = |r + 1e-8| about the axis r / t', which is not a unit vector: with d = sqrt(3) 1e-8 the
# matrix I + sin(t') K + (1 - cos(t')) K^2 differs from exp(r) by at most d (the angle in the sine) + d (the axis length in sin K)
# + 2 . 2 d / pi (the axis length, squared, in the last term, largest at t = pi) < 3.3 d = 5.7e-8 in every entry.  Both sides of the
# identity carry it, with different r, on a lever of at most 1.25 m from the root joint, over three entries of a row:
# 2 . 3 . 5.7e-8 . 1.25 = 4.3e-7 m.  Measured: 2.7e-8 m.  In pixels at fx = 1410 and z >= 2.5 m: 4.3e-7 . 1410 / 2.5.
BODY_EPS_METRES = 4.3e-7
BODY_EPS_PIXELS = 4.3e-7 * 1410 / 2.5

# ---- mp_verts_bounds with a shift: | kernel - float64 | of max_i |v_i + shift_f| over F in {1, 3}, n in {1, 63, 64, 65, 13 780}
# (coordinates up to 9, the norm up to 16.3: an fp32 ulp is 1.9e-6)
BOUNDS_NORM_ABS_MEASURED = 1.127e-06        # F = 3, n = 64
# ---- build_scene on 3 frames x 2 persons (test_build_scene_end_to_end), against the float64 restatement
MAX_HUMAN_SPHERE_ABS_MEASURED = 1.133e-07   # metres, normalize='first_frame' (2.568e-08 per frame); the sphere is 1.0 - 1.1 m
NORMALIZE_TRANS_ABS_MEASURED = 1.217e-07    # metres, per frame (1.091e-07 first frame): the shift comes from fp32 vertex extremes at 3 - 5 m
CAM_REL_MEASURED = 4.602e-08                # | cam_f - float64 | / max | cam_f | per frame
REPROJECTION_PX_MEASURED = 1.468e-05        # the dataset item's bodies against the original camera-space bodies under K, px (of 128)


def bound(measured):
    return MARGIN * measured
