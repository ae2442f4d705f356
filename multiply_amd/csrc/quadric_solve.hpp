// The representative of one cell of the quadric vertex clustering (simplify.hip k_simplify_quadrics), as a __host__ __device__
// routine so that a host program can run it (tests/simplify_host.cpp).  Everything is relative to the cell's centre.
//   quadric_point   A (packed upper triangle xx xy xz yy yz zz of sum n n^T), b (sum n (n . (p0 - c))), the mean of the cell's own
//                   vertices, lam, half = h / 2  ->  x in [-half, half]^3.
//                   trace(A) > 0:  (A + l I) x = b + l mean with l = lam trace(A) / 3, by Cholesky.  A is positive semi-definite
//                   with largest eigenvalue <= trace(A), so the eigenvalues of A + l I lie in [l, trace(A) + l]: the condition
//                   number is at most 3 / lam + 1 whatever the rank of A, every pivot is >= l > 0 up to rounding, and there is
//                   no rank decision to take.  A flat cell (rank 1) moves its point along the plane towards the mean, an edge
//                   cell (rank 2) along the edge, a corner cell (rank 3) sits on the corner.
//                   otherwise (no face, zero-area faces only, or a NaN): x = mean.
//                   Returns 1 when it solved, 0 when it took the mean.  x_free (3, may be null) receives x before the clamp.
// No contraction into fused multiply-adds: the host program, the kernel and the float64 reference of the tests round alike.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__host__ __device__ inline double quadric_clamp(double v, double half) { return v < -half ? -half : (v > half ? half : v); }

__host__ __device__ inline int quadric_point(const double* A, const double* b, const double* mean, double lam, double half,
                                             double* x, double* x_free) {
#pragma clang fp contract(off)
    const double trace = A[0] + A[3] + A[5];
    int solved = 0;
    double y[3] = {mean[0], mean[1], mean[2]};
    if (trace > 0.0 && isfinite(trace)) {
        const double l = lam * trace / 3.0;
        const double m00 = A[0] + l, m01 = A[1], m02 = A[2], m11 = A[3] + l, m12 = A[4], m22 = A[5] + l;
        const double r0 = b[0] + l * mean[0], r1 = b[1] + l * mean[1], r2 = b[2] + l * mean[2];
        // M = L L^T
        const double l00 = sqrt(m00);
        const double l10 = m01 / l00, l20 = m02 / l00;
        const double d1 = m11 - l10 * l10;
        const double l11 = sqrt(d1);
        const double l21 = (m12 - l20 * l10) / l11;
        const double d2 = m22 - l20 * l20 - l21 * l21;
        const double l22 = sqrt(d2);
        if (m00 > 0.0 && d1 > 0.0 && d2 > 0.0) {
            const double z0 = r0 / l00;
            const double z1 = (r1 - l10 * z0) / l11;
            const double z2 = (r2 - l20 * z0 - l21 * z1) / l22;
            const double x2 = z2 / l22;
            const double x1 = (z1 - l21 * x2) / l11;
            const double x0 = (z0 - l10 * x1 - l20 * x2) / l00;
            if (isfinite(x0) && isfinite(x1) && isfinite(x2)) {
                y[0] = x0; y[1] = x1; y[2] = x2;
                solved = 1;
            }
        }
    }
    for (int a = 0; a < 3; ++a) {
        if (x_free) x_free[a] = y[a];
        x[a] = quadric_clamp(y[a], half);
    }
    return solved;
}
