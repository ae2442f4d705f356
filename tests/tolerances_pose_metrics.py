"""Bounds of tests/test_pose_metrics_gpu.py and tests/test_smpl_pose_batch_gpu.py.

SUMS is derived, PROCRUSTES is 4 x a measurement (the margin convention of tolerances_penetration.py), the posing bounds are those
of the existing single-row test (tests/test_geom_gpu.py test_smpl_server)."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)

# plain and root-aligned means, contact-distance means: double sums of at most 6 890 terms on the same float32 inputs in another
# order; n 2^-53 = 7.7e-13 relative for n = 6 890 is the worst case of a sum, the terms themselves (a square root of three squares)
# are off by a few 2^-53.  The image kernels' bound for the same reason (tolerances of tests/test_image_metrics_gpu.py).
SUMS = 1.0e-12

# Procrustes mean: | kernel - restatement | / M, M = the largest |coordinate| of the item's two point sets.  The residual is a
# difference of O(M) numbers (s R p + t against x), so its error is absolute in M whatever the size of the residual itself.  The
# kernel's SVD (one-sided Jacobi) and numpy's (LAPACK) differ in route, so the bound is not derivable: measured on the MI355X over
# the cases of test_pose_errors_against_the_restatement (random, mirrored, coplanar, near-planar clouds; n = 3, 24, 257, 6 890;
# M = 1 and 5 items).  Measured 1.244e-16 (the mirrored three-point item, whose exact residual is 0: the restatement itself returns
# 3.6e-16 there; the items with a residual above 1e-4 stay below 6e-17): both routes are at the rounding of a double.
# The bound that follows is about two ulps of a double at the coordinate scale: a compiler, libm or LAPACK change that moves a
# square root or a fused multiply-add in k_pose_errors or in numpy.linalg.svd can exceed it.  A failure of that size (still ~1e-15)
# means RE-MEASURE on the cases above and record the new value here and in DESIGN 6i; it is not a defect of either route.
PROCRUSTES_MEASURED = 1.244e-16
PROCRUSTES = 4.0 * PROCRUSTES_MEASURED

# mp_smpl_pose_batch against the oracle, row by row: the bounds of test_smpl_server
POSE_POINTS = 5.0e-6          # vertices and joints
POSE_TFS = 2.0e-5             # bone transforms


def coordinate_scale(*arrays):
    """M: the largest finite |coordinate| of the arrays"""
    m = 0.0
    for a in arrays:
        a = np.asarray(a, np.float64)
        a = a[np.isfinite(a)]
        m = max(m, float(np.abs(a).max()) if a.size else 0.0)
    return m


def end_to_end(key, value, M, unit_scale=1.0):
    """pose_metrics against the restatement fed the ORACLE's bodies: the kernels' own bound on the value plus the posing error
    propagated.  Every posed point is within POSE_POINTS of the oracle's on both sides, and moving each of two points by eps moves
    their distance, hence a mean of distances, by at most 2 eps.  The root-aligned values subtract a root that is itself a posed
    point: 4 eps.  The Procrustes value: with the fitted transform held fixed the two perturbations move each residual by at most
    (1 + s) eps ~ 2 eps (s, the fitted scale, is ~1 here); the transform itself also moves with the perturbations.  That second
    part is NOT derived here: it is ASSUMED to be at most another 2 eps (the fit averages the perturbations over 24 or 6 890
    points), which makes 4 eps.  Measured: 2.7e-6 cm against this 2e-3 cm.  A contact distance's ends are a vertex and a convex
    combination of vertices: 2 eps."""
    eps = POSE_POINTS * unit_scale
    if key in ("mpjpe_global", "mve_global", "cd", "cd_gt"):
        return SUMS * abs(value) + 2.0 * eps
    if key in ("mpjpe", "mve"):
        return SUMS * abs(value) + 4.0 * eps
    if key in ("pa_mpjpe", "pa_mve"):
        return PROCRUSTES * M * unit_scale + 4.0 * eps
    raise KeyError(key)
