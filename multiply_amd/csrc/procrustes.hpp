// The 3 x 3 Procrustes routine shared by pose_metrics.hip (k_pose_errors) and registration.hip (k_reg_fit_pairs), with its two
// helpers.  __host__ __device__, so that a host program can run it (tests/procrustes_host.cpp).  The method is described at the
// top of pose_metrics.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

__host__ __device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a unit vector orthogonal to the unit vector a: the coordinate axis least along a, made orthogonal
__host__ __device__ inline void any_orthogonal(const double* a, double* o) {
    const int k = fabs(a[0]) <= fabs(a[1]) ? (fabs(a[0]) <= fabs(a[2]) ? 0 : 2) : (fabs(a[1]) <= fabs(a[2]) ? 1 : 2);
    double e[3] = {0.0, 0.0, 0.0};
    e[k] = 1.0;
    const double d = a[k];
    double nn = 0.0;
    for (int i = 0; i < 3; ++i) { o[i] = e[i] - d * a[i]; nn += o[i] * o[i]; }
    nn = sqrt(nn);
    for (int i = 0; i < 3; ++i) o[i] /= nn;
}

// H [3][3] (row = predicted axis, column = ground-truth axis) -> R (row-major, x ~ R p) and tr(S D)
__host__ __device__ inline void procrustes(const double* H, double* Rm, double& trSD) {
    double A[3][3], Vm[3][3];      // COLUMNS: A[c] = column c of H V, Vm[c] = column c of V
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) { A[c][r] = H[3 * r + c]; Vm[c][r] = r == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
        for (int i = 0; i < 2; ++i)
            for (int j = i + 1; j < 3; ++j) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; ++r) { al += A[i][r] * A[i][r]; be += A[j][r] * A[j][r]; ga += A[i][r] * A[j][r]; }
                if (ga == 0.0 || fabs(ga) <= 1e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
                for (int r = 0; r < 3; ++r) {
                    const double x = A[i][r], y = A[j][r];
                    A[i][r] = cs * x - sn * y;
                    A[j][r] = sn * x + cs * y;
                    const double p = Vm[i][r], q = Vm[j][r];
                    Vm[i][r] = cs * p - sn * q;
                    Vm[j][r] = sn * p + cs * q;
                }
            }
        if (!rotated) break;
    }
    double sg[3];
    int ord[3] = {0, 1, 2};
    for (int c = 0; c < 3; ++c) sg[c] = sqrt(A[c][0] * A[c][0] + A[c][1] * A[c][1] + A[c][2] * A[c][2]);
    for (int a = 0; a < 2; ++a)                     // sort downwards (ties keep their order)
        for (int b = 0; b < 2 - a; ++b)
            if (sg[ord[b]] < sg[ord[b + 1]]) { const int x = ord[b]; ord[b] = ord[b + 1]; ord[b + 1] = x; }
    const double s1 = sg[ord[0]], s2 = sg[ord[1]], s3 = sg[ord[2]];
    const double *v1 = Vm[ord[0]], *v2 = Vm[ord[1]];
    double u1[3], u2[3], u3[3], v3[3];
    if (s1 > 0.0) {
        for (int r = 0; r < 3; ++r) u1[r] = A[ord[0]][r] / s1;
    } else {                                        // H = 0: any rotation is optimal (s = 0 makes it irrelevant)
        u1[0] = v1[0]; u1[1] = v1[1]; u1[2] = v1[2];
    }
    if (s2 > 1e-14 * s1) {
        double d = 0.0, nn = 0.0;                   // one Gram-Schmidt step: u2 is orthogonal to u1 only to eps S_1 / S_2
        for (int r = 0; r < 3; ++r) { u2[r] = A[ord[1]][r] / s2; d += u2[r] * u1[r]; }
        for (int r = 0; r < 3; ++r) { u2[r] -= d * u1[r]; nn += u2[r] * u2[r]; }
        nn = sqrt(nn);
        for (int r = 0; r < 3; ++r) u2[r] /= nn;
    } else if (s1 > 0.0) {                          // collinear: the rotation about the line is free
        any_orthogonal(u1, u2);
    } else {
        u2[0] = v2[0]; u2[1] = v2[1]; u2[2] = v2[2];
    }
    cross3(u1, u2, u3);
    cross3(v1, v2, v3);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Rm[3 * a + b] = v1[a] * u1[b] + v2[a] * u2[b] + v3[a] * u3[b];
    double hv[3], dot = 0.0;                        // H v3' = +- S_3 u3: the sign is D_3's
    for (int r = 0; r < 3; ++r) hv[r] = H[3 * r] * v3[0] + H[3 * r + 1] * v3[1] + H[3 * r + 2] * v3[2];
    for (int r = 0; r < 3; ++r) dot += hv[r] * u3[r];
    trSD = s1 + s2 + (dot < 0.0 ? -s3 : s3);
}
