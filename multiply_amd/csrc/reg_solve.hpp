// One Gauss-Newton step of the point-to-plane registration (registration.hip k_reg_step), as a __host__ __device__ routine so
// that a host program can run it (tests/registration_host.cpp).  Layouts: include/multiply_hip.h MP_REG_*.
//   unknowns   delta = [omega (3), v (3), sigma]: the update x -> c + exp(sigma) exp([omega]x) (x - c) + v about the fixed origin c.
//              A pair's row is a = [(x - c) x n, n, (x - c) . n] with residual r = (x - q) . n, linearised r' = r + a . delta.
//   reg_solve  A delta = b for the leading m x m block (m = 6 rigid, 7 similarity) of the packed upper triangle: Cholesky
//              A = L L^T, then ONE step of iterative refinement with the residual b - A delta (a 7 x 7 costs nothing; it takes the
//              error from ~m cond(A) 2^-53 to a small multiple of cond(A) 2^-53).  A pivot that is not above 2^-40 of its diagonal
//              entry counts as non-positive: it has lost 40 of its 53 bits to cancellation, the matrix is singular to working
//              precision.  The ratio does not change under a diagonal scaling D A D, so an ill-scaled system is no special case.
//   reg_step   sums (one slot, MP_REG_SLOT doubles, already added over the slots) -> the new state: solve, compose, RMS, tau2,
//              step size, flag.  Returns the flag.  Fewer than 7 accepted pairs or a failed solve: MP_REG_DEGENERATE, the
//              transform stays as it was.  delta (7, may be null) receives the solution (0 where there is none).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/multiply_hip.h"

__host__ __device__ inline int reg_tri(int i, int j) { return i * 7 - i * (i - 1) / 2 + (j - i); }     // i <= j < 7

__host__ __device__ inline bool reg_solve(const double* tri, const double* b, int m, double* x) {
    double A[7][7], L[7][7];
    for (int i = 0; i < m; ++i)
        for (int j = i; j < m; ++j) A[i][j] = A[j][i] = tri[reg_tri(i, j)];
    const double lost = 9.094947017729282e-13;      // 2^-40
    for (int j = 0; j < m; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > lost * A[j][j]) || !isfinite(d)) return false;       // also NaN and a zero diagonal
        const double l = sqrt(d);
        L[j][j] = l;
        for (int i = j + 1; i < m; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / l;
        }
    }
    double rhs[7], y[7];
    for (int i = 0; i < m; ++i) { rhs[i] = b[i]; x[i] = 0.0; }
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i < m; ++i) {
            double v = rhs[i];
            for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
            y[i] = v / L[i][i];
        }
        for (int i = m - 1; i >= 0; --i) {
            double v = y[i];
            for (int k = i + 1; k < m; ++k) v -= L[k][i] * y[k];
            y[i] = v / L[i][i];
        }
        for (int i = 0; i < m; ++i) x[i] += y[i];
        for (int i = 0; i < m; ++i) {               // the residual of the refined solution
            double v = b[i];
            for (int k = 0; k < m; ++k) v -= A[i][k] * x[k];
            rhs[i] = v;
        }
    }
    for (int i = 0; i < m; ++i)
        if (!isfinite(x[i])) return false;
    return true;
}

// x = s R p + t of a state block
__host__ __device__ inline void reg_apply_fwd(const double* st, const double* p, double* x) {
    const double s = st[MP_REG_S];
    const double* R = st + MP_REG_R;
    for (int a = 0; a < 3; ++a) x[a] = s * (R[3 * a] * p[0] + R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2]) + st[MP_REG_T + a];
}

__host__ __device__ inline int reg_step(const double* sums, int similarity, double reject, double tol, double* st, double* delta) {
    if (delta)
        for (int i = 0; i < 7; ++i) delta[i] = 0.0;
    if (st[MP_REG_FLAG] != 0.0) return (int)st[MP_REG_FLAG];
    const double acc = sums[MP_REG_SLOT_ACCEPTED];
    st[MP_REG_ACCEPTED] = acc;
    st[MP_REG_REJECTED] = sums[MP_REG_SLOT_REJECTED];
    st[MP_REG_LEFT_OUT] = sums[MP_REG_SLOT_LEFT_OUT];
    const double rms = acc > 0.0 ? sqrt(sums[MP_REG_SLOT_D2] / acc) : 0.0;
    st[MP_REG_RMS] = rms;
    st[MP_REG_RMS_PLANE] = acc > 0.0 ? sqrt(sums[MP_REG_SLOT_R2] / acc) : 0.0;
    const int m = similarity ? 7 : 6;
    double b[7], d[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 7; ++i) b[i] = -sums[MP_REG_SLOT_ATR + i];
    if (acc < 7.0 || !reg_solve(sums + MP_REG_SLOT_ATA, b, m, d)) {
        st[MP_REG_FLAG] = (double)MP_REG_DEGENERATE;
        st[MP_REG_STEP] = 0.0;
        return MP_REG_DEGENERATE;
    }
    if (delta)
        for (int i = 0; i < m; ++i) delta[i] = d[i];
    // exp([omega]x) by Rodrigues: I + a K + b K^2, a = sin th / th, b = (1 - cos th) / th^2 = (sin(th/2) / (th/2))^2 / 2
    const double th = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), h = 0.5 * th;
    const double ca = th > 0.0 ? sin(th) / th : 1.0, sh = h > 0.0 ? sin(h) / h : 1.0, cb = 0.5 * sh * sh;
    const double K[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double k2 = 0.0;
            for (int k = 0; k < 3; ++k) k2 += K[3 * i + k] * K[3 * k + j];
            E[3 * i + j] = (i == j ? 1.0 : 0.0) + ca * K[3 * i + j] + cb * k2;
        }
    const double es = similarity ? exp(d[6]) : 1.0;
    double nw[MP_REG_STATE];
    for (int i = 0; i < MP_REG_STATE; ++i) nw[i] = st[i];
    nw[MP_REG_S] = st[MP_REG_S] * es;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += E[3 * i + k] * st[MP_REG_R + 3 * k + j];
            nw[MP_REG_R + 3 * i + j] = v;
        }
    double tc[3];
    for (int a = 0; a < 3; ++a) tc[a] = st[MP_REG_T + a] - st[MP_REG_C + a];
    for (int a = 0; a < 3; ++a)
        nw[MP_REG_T + a] = st[MP_REG_C + a] + es * (E[3 * a] * tc[0] + E[3 * a + 1] * tc[1] + E[3 * a + 2] * tc[2]) + d[3 + a];
    // step size: the largest displacement of the 8 corners of the target's bounding box
    double step = 0.0, diag = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double e = st[MP_REG_BOX_HI + a] - st[MP_REG_BOX_LO + a];
        diag += e * e;
    }
    diag = sqrt(diag);
    for (int k = 0; k < 8; ++k) {
        double p[3], x0[3], x1[3];
        for (int a = 0; a < 3; ++a) p[a] = (k >> a) & 1 ? st[MP_REG_BOX_HI + a] : st[MP_REG_BOX_LO + a];
        reg_apply_fwd(st, p, x0);
        reg_apply_fwd(nw, p, x1);
        const double e = sqrt((x1[0] - x0[0]) * (x1[0] - x0[0]) + (x1[1] - x0[1]) * (x1[1] - x0[1]) + (x1[2] - x0[2]) * (x1[2] - x0[2]));
        step = e > step ? e : step;
    }
    if (!isfinite(step) || !(nw[MP_REG_S] > 0.0) || !isfinite(nw[MP_REG_S])) {
        st[MP_REG_FLAG] = (double)MP_REG_DEGENERATE;
        st[MP_REG_STEP] = 0.0;
        return MP_REG_DEGENERATE;
    }
    for (int i = 0; i < MP_REG_T + 3; ++i) st[i] = nw[i];
    st[MP_REG_TAU2] = reject > 0.0 ? (reject * rms) * (reject * rms) : (double)INFINITY;
    st[MP_REG_ITERS] += 1.0;
    st[MP_REG_STEP] = step;
    if (step <= tol * diag) st[MP_REG_FLAG] = (double)MP_REG_CONVERGED;
    return (int)st[MP_REG_FLAG];
}
