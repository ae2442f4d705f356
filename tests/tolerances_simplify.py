"""Bounds of the simplification tests, derived from the arithmetic, not tuned.

The kernel and the float64 reference (tests/mesh_simplify_reference.py) form every contribution with the same operations in
the same order and without fused multiply-adds, so a contribution has the same bits on both sides; what differs is the ORDER in which
a cell's contributions are added (16 lanes and a butterfly against numpy's sequential add.at), the solver (Cholesky against LAPACK's
LU) and the final rounding, which only the kernel does.

  sums      a sum of m terms in any order differs from the exact sum by at most (m - 1) u sum|terms|, u = 2^-53; two orders differ
            by twice that.  For A the terms of a diagonal entry are positive, so sum|terms| <= trace(A); the off-diagonal entries
            obey |n_i n_j| <= (n_i^2 + n_j^2) / 2.  For b, |n (n . d)| <= |n|^2 |d| <= |n|^2 D with D the largest |p0 - c| of the
            segment.  So |dA| <= 2 m u trace(A) and |db| <= 2 m u trace(A) D, and the mean (k vertices inside the cell) moves by at
            most 2 k u h.
  solve     (A + l I) x = b + l mean with l = lam trace(A) / 3:  |(A + l I)^-1| = 1 / l' <= 3 / (lam trace(A)), hence
            |dx| <= (3 / lam) (2 m u) (D + |x|) + 2 k u h from the sums, plus the solvers' own error, each at most
            16 u cond |x| with cond <= 3 / lam + 1 (a 3 x 3 Cholesky or LU: 10 u cond, and 6 u for forming l, the diagonal and the
            right-hand side).  Together at most  2 (3 / lam + 1) (m + k + 16) u (h + D + |x|);  `reach` = D + |x| comes from the
            reference, |x| taken BEFORE the clamp (the clamp is 1-Lipschitz).
  position  c + x is formed in double on both sides (2 u |coordinate| each) and rounded once to float32 by the kernel: half a float32
            ulp of the largest |coordinate|.
"""
import numpy as np

U = 2.0 ** -53
SOLVER = 16.0          # u cond |x| of one 3 x 3 solve including the formation of the system (above)


def half_ulp32(x):
    return 0.5 * float(np.spacing(np.float32(abs(float(x)))))


def condition(lam):
    return 3.0 / lam + 1.0


def double_part(seg, n_verts, reach, h, lam):
    """the part of the position bound that is double-precision error (per output vertex; arrays broadcast)"""
    return 2.0 * condition(lam) * (np.asarray(seg, np.float64) + np.asarray(n_verts, np.float64) + SOLVER) * U * (h + np.asarray(reach, np.float64))


def position_bound(coord_max, seg, n_verts, reach, h, lam):
    return half_ulp32(coord_max) + 4.0 * U * coord_max + double_part(seg, n_verts, reach, h, lam)


def attr_bound(attr_max, n_verts):
    """a mean of k float32 values in double, rounded once: half a float32 ulp plus the two orders' (k - 1) u each"""
    return half_ulp32(attr_max) + 2.0 * (np.asarray(n_verts, np.float64) + 1.0) * U * attr_max


def solve_bound(lam):
    """relative bound |x - x_lapack| / |x| of the host solve against numpy's on the same system: both solvers' errors"""
    return 2.0 * SOLVER * condition(lam) * U
