// Pose metrics (multiply_amd/pose_metrics.py): the means MPJPE / MVE are made of, and the contact distance.
//   k_pose_errors     one workgroup of 256 threads per item (one person of one frame: n joints or vertices, predicted and ground
//                     truth).  Pass 1: the two means, the plain and the root-aligned distance sums, the non-finite count; pass 2:
//                     H = sum (p - mean p)(x - mean x)^T and sum |p - mean p|^2 about those means (no cancellation); thread 0 then
//                     solves the 3 x 3 Procrustes problem; pass 3: the residual sum.  The points are read from global memory each
//                     time (at n = 6 890 the two sets are 165 KB: passes 2 and 3 come out of the L2).  Everything after the loads
//                     is double; a thread adds the points t, t + 256, ... in order, the lanes go through the xor butterfly, the
//                     four waves are added in order: the same bits on every call.
//   procrustes        (in procrustes.hpp, shared with registration.hip)
//                     H = U S V^T by one-sided Jacobi rotations of H's columns (H V = U S: no H^T H, so small singular values
//                     keep their relative accuracy), singular values sorted downwards.  The rotation needs no third singular
//                     vector: with u3' = u1 x u2 and v3' = v1 x v2, V diag(1, 1, sign det(V U^T)) U^T = v1 u1^T + v2 u2^T +
//                     v3' u3'^T whatever sign the SVD gave u3 and v3 -- a coplanar cloud (S_3 = 0) or a mirrored one (D_3 = -1)
//                     is no special case.  tr(S D) = S_1 + S_2 + sign S_3, the sign that of (H v3') . u3'.
//   k_contact_frame   one workgroup per frame over that frame's correspondences (sorted by frame on the host), the distance in
//                     double, the frame's sum -> work[frame]; k_contact_finish adds the frames in order.
// No atomics.  Entry points: include/multiply_hip.h mp_pose_errors, mp_contact_distance.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/multiply_hip.h"
#include "procrustes.hpp"

namespace {

constexpr int TB = 256;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sums of K doubles per thread, left in v[] of EVERY thread: lanes by the xor butterfly, then the waves in order
template <int K>
__device__ __forceinline__ void block_sums(double* v, double (*sh)[K]) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double s = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double t = 0.0;
        for (int w = 0; w < TB / 64; ++w) t += sh[w][j];
        v[j] = t;
    }
}

__global__ __launch_bounds__(TB) void k_pose_errors(const float* __restrict__ pred, const float* __restrict__ gt,
                                                    const float* __restrict__ pred_root, const float* __restrict__ gt_root,
                                                    int n, double* __restrict__ out) {
    __shared__ double sh[TB / 64][10];
    __shared__ double tr[12];                       // s R [9], t [3]
    const int t = threadIdx.x;
    const size_t m = blockIdx.x;
    const float* P = pred + m * (size_t)n * 3;
    const float* X = gt + m * (size_t)n * 3;
    const bool roots = pred_root != nullptr;
    double dr[3] = {0.0, 0.0, 0.0};                 // gt_root - pred_root
    double bad = 0.0;
    if (roots)
        for (int a = 0; a < 3; ++a) {
            const double rp = pred_root[3 * m + a], rx = gt_root[3 * m + a];
            if (!isfinite(rp) || !isfinite(rx)) bad = 1.0;     // every thread sees it; counted once below
            dr[a] = rx - rp;
        }
    double s[10];
    for (int j = 0; j < 10; ++j) s[j] = 0.0;
    if (t != 0) bad = 0.0;
    const double p0[3] = {P[0], P[1], P[2]};        // do the predicted points all coincide?  (their spread is then 0 exactly;
                                                    // the sum about a rounded mean need not be)
    for (int i = t; i < n; i += TB) {
        double p[3], x[3], e[3];
        bool fin = true;
        for (int a = 0; a < 3; ++a) {
            p[a] = P[3 * (size_t)i + a];
            x[a] = X[3 * (size_t)i + a];
            fin = fin && isfinite(p[a]) && isfinite(x[a]);
            e[a] = p[a] - x[a];
        }
        if (!fin) { bad += 1.0; continue; }
        if (p[0] != p0[0] || p[1] != p0[1] || p[2] != p0[2]) s[9] += 1.0;
        for (int a = 0; a < 3; ++a) { s[a] += p[a]; s[3 + a] += x[a]; }
        s[6] += sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        for (int a = 0; a < 3; ++a) e[a] += dr[a];  // (p - rp) - (x - rx)
        s[7] += sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    }
    s[8] = bad;
    block_sums<10>(s, sh);
    double* o = out + 4 * m;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (s[8] > 0.0) {                               // uniform over the workgroup: s[] holds the same sums in every thread
        if (t == 0) { o[0] = nan; o[1] = nan; o[2] = nan; o[3] = 1.0; }
        return;
    }
    const double inv = 1.0 / (double)n;
    double mp_[3], mx[3];
    for (int a = 0; a < 3; ++a) { mp_[a] = s[a] * inv; mx[a] = s[3 + a] * inv; }
    const double plain = s[6] * inv, aligned = roots ? s[7] * inv : nan;
    const bool coincide = s[9] == 0.0;
    for (int j = 0; j < 10; ++j) s[j] = 0.0;
    for (int i = t; i < n; i += TB) {
        double p[3], x[3];
        for (int a = 0; a < 3; ++a) { p[a] = (double)P[3 * (size_t)i + a] - mp_[a]; x[a] = (double)X[3 * (size_t)i + a] - mx[a]; }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) s[3 * a + b] += p[a] * x[b];
        s[9] += p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    }
    block_sums<10>(s, sh);
    if (coincide || s[9] == 0.0) {                  // every predicted point coincides: no scale
        if (t == 0) { o[0] = plain; o[1] = aligned; o[2] = nan; o[3] = 2.0; }
        return;
    }
    if (plain == 0.0) {                             // the two sets are equal: the identity attains the minimum, 0, exactly
        if (t == 0) { o[0] = plain; o[1] = aligned; o[2] = 0.0; o[3] = 0.0; }
        return;
    }
    if (t == 0) {
        double Rm[9], trSD;
        procrustes(s, Rm, trSD);
        const double sc = trSD / s[9];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) tr[3 * a + b] = sc * Rm[3 * a + b];
            tr[9 + a] = mx[a] - sc * (Rm[3 * a] * mp_[0] + Rm[3 * a + 1] * mp_[1] + Rm[3 * a + 2] * mp_[2]);
        }
    }
    __syncthreads();
    double r[1] = {0.0};
    for (int i = t; i < n; i += TB) {
        double p[3], e[3];
        for (int a = 0; a < 3; ++a) p[a] = P[3 * (size_t)i + a];
        for (int a = 0; a < 3; ++a)
            e[a] = tr[3 * a] * p[0] + tr[3 * a + 1] * p[1] + tr[3 * a + 2] * p[2] + tr[9 + a] - (double)X[3 * (size_t)i + a];
        r[0] += sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    }
    block_sums<1>(r, reinterpret_cast<double(*)[1]>(&sh[0][0]));
    if (t == 0) { o[0] = plain; o[1] = aligned; o[2] = r[0] * inv; o[3] = 0.0; }
}

__global__ __launch_bounds__(TB) void k_contact_frame(const float* __restrict__ verts, int F, int P, int V,
                                                      const int* __restrict__ faces, int n_faces, const int* __restrict__ corr,
                                                      const float* __restrict__ bary, const int* __restrict__ frame_start, int m,
                                                      double* __restrict__ work, double* __restrict__ out) {
    __shared__ double sh[TB / 64][1];
    const int f = blockIdx.x, t = threadIdx.x;
    const int lo = max(0, min(frame_start[f], m)), hi = max(lo, min(frame_start[f + 1], m));
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double s[1] = {0.0};
    for (int i = lo + t; i < hi; i += TB) {
        const int* c = corr + 5 * (size_t)i;
        const int a = c[1], va = c[2], b = c[3], fb = c[4];
        double d = nan;
        if (c[0] == f && a >= 0 && a < P && b >= 0 && b < P && va >= 0 && va < V && fb >= 0 && fb < n_faces) {
            const int k0 = faces[3 * fb], k1 = faces[3 * fb + 1], k2 = faces[3 * fb + 2];
            if (k0 >= 0 && k0 < V && k1 >= 0 && k1 < V && k2 >= 0 && k2 < V) {
                const float* pa = verts + (((size_t)f * P + a) * V + va) * 3;
                const float* qb = verts + ((size_t)f * P + b) * V * 3;
                const double w0 = bary[3 * (size_t)i], w1 = bary[3 * (size_t)i + 1], w2 = bary[3 * (size_t)i + 2];
                double e2 = 0.0;
                for (int x = 0; x < 3; ++x) {
                    const double q = w0 * (double)qb[3 * (size_t)k0 + x] + w1 * (double)qb[3 * (size_t)k1 + x] +
                                     w2 * (double)qb[3 * (size_t)k2 + x];
                    const double e = (double)pa[x] - q;
                    e2 += e * e;
                }
                d = sqrt(e2);
            }
        }
        s[0] += d;
    }
    block_sums<1>(s, sh);
    if (t == 0) {
        work[f] = s[0];
        out[2 + f] = hi > lo ? s[0] / (double)(hi - lo) : nan;
        out[2 + F + f] = (double)(hi - lo);
    }
}

// out [2 + 2 F]: reads the per-frame counts k_contact_frame left at out[2 + F ..], writes out[0], out[1]
__global__ __launch_bounds__(TB) void k_contact_finish(const double* __restrict__ work, int F, double* out) {
    __shared__ double sh[TB / 64][2];
    double s[2] = {0.0, 0.0};
    for (int f = threadIdx.x; f < F; f += TB) { s[0] += work[f]; s[1] += out[2 + F + f]; }
    block_sums<2>(s, sh);
    if (threadIdx.x == 0) {
        out[0] = s[1] > 0.0 ? s[0] / s[1] : __longlong_as_double(0x7ff8000000000000LL);
        out[1] = s[1];
    }
}
}  // namespace

extern "C" int mp_pose_errors(const float* pred, const float* gt, const float* pred_root, const float* gt_root, int M, int n,
                              double* out, void* stream) {
    if (M < 0 || n < 1 || (pred_root == nullptr) != (gt_root == nullptr)) return -1;
    if (M == 0) return 0;
    if (!pred || !gt || !out) return -1;
    hipLaunchKernelGGL(k_pose_errors, dim3(M), dim3(TB), 0, (hipStream_t)stream, pred, gt, pred_root, gt_root, n, out);
    return (int)hipGetLastError();
}

extern "C" int mp_contact_distance(const float* verts, int F, int P, int V, const int* faces, int n_faces, const int* corr,
                                   const float* bary, const int* frame_start, int m, double* work, double* out, void* stream) {
    if (F < 1 || P < 1 || V < 1 || n_faces < 1 || m < 0 || !verts || !faces || !frame_start || !work || !out) return -1;
    if (m > 0 && (!corr || !bary)) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_contact_frame, dim3(F), dim3(TB), 0, st, verts, F, P, V, faces, n_faces, corr, bary, frame_start, m, work,
                       out);
    hipLaunchKernelGGL(k_contact_finish, dim3(1), dim3(TB), 0, st, work, F, out);
    return (int)hipGetLastError();
}
