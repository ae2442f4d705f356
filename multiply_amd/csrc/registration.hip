// Registration of meshes before the mesh metrics (multiply_amd/registration.py): point-to-plane ICP for x = s R p + t on
// closest-surface correspondences, and the closed form for explicit pairs.  State and slot layouts: include/multiply_hip.h.
//   k_reg_apply       one thread per point: the transform (or its inverse) in double, rounded once to fp32.
//   k_reg_rows        one direction's pairs -> the sums of the normal equations.  A thread keeps the 40 sums of a slot in double
//                     registers over its pairs (b 256 + t + k G 256, ascending), the lanes go through the xor butterfly, the four
//                     waves are added in order, the workgroup's sums go to work[b]; k_reg_rows_finish (one workgroup, thread j
//                     owns sum j) adds the G partial sums in ascending order into the slot.  48 B in per pair, 40 fused
//                     multiply-adds: bound by the loads' latency at the 10^4..10^5 pairs of a call, beside a closest query
//                     that costs ~100 flops per pair AND FACE.
//   k_reg_step        one workgroup: thread j adds sum j over the slots in ascending order, thread 0 runs reg_step
//                     (reg_solve.hpp: Cholesky, Rodrigues, the new state).
//   k_reg_fit_pairs   one workgroup, the passes and the order of k_pose_errors (pose_metrics.hip) with weights; thread 0 runs
//                     procrustes (procrustes.hpp).
// Once the state's flag is set k_reg_rows / _finish / k_reg_step return at once: no host synchronisation is needed to stop.
// No atomics.  Entry points: mp_reg_apply, mp_reg_rows, mp_reg_step, mp_reg_fit_pairs.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/multiply_hip.h"
#include "procrustes.hpp"
#include "reg_solve.hpp"

namespace {

constexpr int TB = 256, NS = MP_REG_SLOT;

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

__global__ __launch_bounds__(TB) void k_reg_apply(const float* p, int n, const double* __restrict__ st, int inverse, float* out) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const double s = st[MP_REG_S];
    const double* R = st + MP_REG_R;
    const double* T = st + MP_REG_T;
    const double x[3] = {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
    double y[3];
    if (!inverse) {
        for (int a = 0; a < 3; ++a) y[a] = s * (R[3 * a] * x[0] + R[3 * a + 1] * x[1] + R[3 * a + 2] * x[2]) + T[a];
    } else {
        const double d[3] = {x[0] - T[0], x[1] - T[1], x[2] - T[2]};
        for (int a = 0; a < 3; ++a) y[a] = (R[a] * d[0] + R[3 + a] * d[1] + R[6 + a] * d[2]) / s;
    }
    for (int a = 0; a < 3; ++a) out[3 * (size_t)i + a] = (float)y[a];
}

__global__ __launch_bounds__(TB) void k_reg_rows(const float* __restrict__ p, const float* __restrict__ q,
                                                 const float* __restrict__ nrm, const int* __restrict__ face, int n_faces,
                                                 int in_source, int n, const double* __restrict__ st, double* __restrict__ work,
                                                 unsigned char* __restrict__ mask) {
    __shared__ double sh[TB / 64][NS];
    if (st[MP_REG_FLAG] != 0.0) return;             // uniform over the grid
    const double s = st[MP_REG_S], tau2 = st[MP_REG_TAU2];
    double R[9], T[3], c[3];
    for (int a = 0; a < 9; ++a) R[a] = st[MP_REG_R + a];
    for (int a = 0; a < 3; ++a) { T[a] = st[MP_REG_T + a]; c[a] = st[MP_REG_C + a]; }
    double v[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) v[j] = 0.0;
    for (size_t i = (size_t)blockIdx.x * TB + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * TB) {
        double pp[3], qq[3], nn[3] = {NAN, NAN, NAN};
        for (int a = 0; a < 3; ++a) { pp[a] = p[3 * i + a]; qq[a] = q[3 * i + a]; }
        if (face) {
            const int f = face[i];
            if (f >= 0 && f < n_faces)
                for (int a = 0; a < 3; ++a) nn[a] = nrm[3 * (size_t)f + a];
        } else {
            for (int a = 0; a < 3; ++a) nn[a] = nrm[3 * i + a];
        }
        if (in_source) {
            const double m[3] = {nn[0], nn[1], nn[2]};
            for (int a = 0; a < 3; ++a) nn[a] = R[3 * a] * m[0] + R[3 * a + 1] * m[1] + R[3 * a + 2] * m[2];
        }
        double x[3], e[3], d2 = 0.0;
        bool fin = true;
        for (int a = 0; a < 3; ++a) {
            x[a] = s * (R[3 * a] * pp[0] + R[3 * a + 1] * pp[1] + R[3 * a + 2] * pp[2]) + T[a];
            e[a] = x[a] - qq[a];
            d2 += e[a] * e[a];
            fin = fin && isfinite(nn[a]);
        }
        fin = fin && isfinite(d2);                  // d2 is finite only if every coordinate of p and q (and the transform) is
        if (!fin) {
            v[MP_REG_SLOT_LEFT_OUT] += 1.0;
            if (mask) mask[i] = 2;
            continue;
        }
        if (d2 > tau2) {
            v[MP_REG_SLOT_REJECTED] += 1.0;
            if (mask) mask[i] = 1;
            continue;
        }
        if (mask) mask[i] = 0;
        double row[7], xc[3] = {x[0] - c[0], x[1] - c[1], x[2] - c[2]};
        cross3(xc, nn, row);
        row[3] = nn[0]; row[4] = nn[1]; row[5] = nn[2];
        row[6] = xc[0] * nn[0] + xc[1] * nn[1] + xc[2] * nn[2];
        const double r = e[0] * nn[0] + e[1] * nn[1] + e[2] * nn[2];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a)
#pragma unroll
            for (int b = a; b < 7; ++b) v[k++] += row[a] * row[b];
#pragma unroll
        for (int a = 0; a < 7; ++a) v[MP_REG_SLOT_ATR + a] += row[a] * r;
        v[MP_REG_SLOT_R2] += r * r;
        v[MP_REG_SLOT_D2] += d2;
        v[MP_REG_SLOT_ACCEPTED] += 1.0;
    }
    block_sums<NS>(v, sh);
    if (threadIdx.x < NS) {
        double mine = 0.0;
#pragma unroll
        for (int j = 0; j < NS; ++j) mine = threadIdx.x == j ? v[j] : mine;     // (no dynamic index into the registers)
        work[(size_t)blockIdx.x * NS + threadIdx.x] = mine;
    }
}

__global__ __launch_bounds__(64) void k_reg_rows_finish(const double* __restrict__ work, int n_blocks, const double* __restrict__ st,
                                                        double* __restrict__ slot) {
    if (st[MP_REG_FLAG] != 0.0 || threadIdx.x >= NS) return;
    double t = 0.0;
    for (int b = 0; b < n_blocks; ++b) t += work[(size_t)b * NS + threadIdx.x];
    slot[threadIdx.x] = t;
}

__global__ __launch_bounds__(64) void k_reg_step(const double* __restrict__ slots, int n_slots, int similarity, double reject,
                                                 double tol, double* st) {
    __shared__ double sums[NS];
    if (st[MP_REG_FLAG] != 0.0) return;
    if (threadIdx.x < NS) {
        double t = 0.0;
        for (int k = 0; k < n_slots; ++k) t += slots[(size_t)k * NS + threadIdx.x];
        sums[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double loc[NS], state[MP_REG_STATE];
        for (int j = 0; j < NS; ++j) loc[j] = sums[j];
        for (int j = 0; j < MP_REG_STATE; ++j) state[j] = st[j];
        reg_step(loc, similarity, reject, tol, state, nullptr);
        for (int j = 0; j < MP_REG_STATE; ++j) st[j] = state[j];
    }
}

__global__ __launch_bounds__(TB) void k_reg_fit_pairs(const float* __restrict__ P, const float* __restrict__ Q,
                                                      const float* __restrict__ W, int n, int similarity, double* __restrict__ out) {
    __shared__ double sh[TB / 64][10];
    const int t = threadIdx.x;
    double s[10];
    for (int j = 0; j < 10; ++j) s[j] = 0.0;
    for (int i = t; i < n; i += TB) {
        double p[3], x[3];
        const double w = W ? (double)W[i] : 1.0;
        bool ok = w > 0.0 && isfinite(w);
        for (int a = 0; a < 3; ++a) {
            p[a] = P[3 * (size_t)i + a];
            x[a] = Q[3 * (size_t)i + a];
            ok = ok && isfinite(p[a]) && isfinite(x[a]);
        }
        if (!ok) { s[7] += 1.0; continue; }
        for (int a = 0; a < 3; ++a) { s[a] += w * p[a]; s[3 + a] += w * x[a]; }
        s[6] += w;
    }
    block_sums<10>(s, sh);
    const double sw = s[6], left = s[7];
    if (!(sw > 0.0)) {                              // uniform: s[] holds the same sums in every thread
        if (t == 0) {
            out[0] = 1.0;
            for (int a = 0; a < 9; ++a) out[1 + a] = a % 4 == 0 ? 1.0 : 0.0;
            out[10] = out[11] = out[12] = 0.0;
            out[13] = 0.0; out[14] = left; out[15] = 1.0;
        }
        return;
    }
    double mp_[3], mx[3];
    for (int a = 0; a < 3; ++a) { mp_[a] = s[a] / sw; mx[a] = s[3 + a] / sw; }
    for (int j = 0; j < 10; ++j) s[j] = 0.0;
    for (int i = t; i < n; i += TB) {
        double p[3], x[3];
        const double w = W ? (double)W[i] : 1.0;
        bool ok = w > 0.0 && isfinite(w);
        for (int a = 0; a < 3; ++a) {
            p[a] = (double)P[3 * (size_t)i + a] - mp_[a];
            x[a] = (double)Q[3 * (size_t)i + a] - mx[a];
            ok = ok && isfinite(p[a]) && isfinite(x[a]);
        }
        if (!ok) continue;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) s[3 * a + b] += w * p[a] * x[b];
        s[9] += w * (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    }
    block_sums<10>(s, sh);
    if (t == 0) {
        double Rm[9], trSD;
        procrustes(s, Rm, trSD);
        const bool spread = s[9] > 0.0;
        const double sc = similarity && spread ? trSD / s[9] : 1.0;
        out[0] = sc;
        for (int a = 0; a < 9; ++a) out[1 + a] = Rm[a];
        for (int a = 0; a < 3; ++a) out[10 + a] = mx[a] - sc * (Rm[3 * a] * mp_[0] + Rm[3 * a + 1] * mp_[1] + Rm[3 * a + 2] * mp_[2]);
        out[13] = sw; out[14] = left; out[15] = spread ? 0.0 : 2.0;
    }
}
}  // namespace

extern "C" int mp_reg_apply(const float* p, int n, const double* state, int inverse, float* out, void* stream) {
    if (n < 0 || !state || (n > 0 && (!p || !out))) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_reg_apply, dim3((n + TB - 1) / TB), dim3(TB), 0, (hipStream_t)stream, p, n, state, inverse, out);
    return (int)hipGetLastError();
}

extern "C" int mp_reg_rows(const float* p, const float* q, const float* normals, const int* face, int n_faces,
                           int normals_in_source, int n, const double* state, double* work, double* slot, unsigned char* mask,
                           void* stream) {
    if (n < 0 || !state || !work || !slot || (n > 0 && (!p || !q || !normals)) || (face && n_faces < 1)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const int G = n == 0 ? 0 : ((n + TB - 1) / TB < MP_REG_MAX_BLOCKS ? (n + TB - 1) / TB : MP_REG_MAX_BLOCKS);
    if (G > 0)
        hipLaunchKernelGGL(k_reg_rows, dim3(G), dim3(TB), 0, st, p, q, normals, face, n_faces, normals_in_source, n, state, work,
                           mask);
    hipLaunchKernelGGL(k_reg_rows_finish, dim3(1), dim3(64), 0, st, work, G, state, slot);
    return (int)hipGetLastError();
}

extern "C" int mp_reg_step(const double* slots, int n_slots, int similarity, double reject, double tol, double* state,
                           void* stream) {
    if (!slots || n_slots < 1 || !state || !(reject >= 0.0) || !(tol >= 0.0)) return -1;
    hipLaunchKernelGGL(k_reg_step, dim3(1), dim3(64), 0, (hipStream_t)stream, slots, n_slots, similarity, reject, tol, state);
    return (int)hipGetLastError();
}

extern "C" int mp_reg_fit_pairs(const float* p, const float* q, const float* w, int n, int similarity, double* out, void* stream) {
    if (n < 0 || !out || (n > 0 && (!p || !q))) return -1;
    hipLaunchKernelGGL(k_reg_fit_pairs, dim3(1), dim3(TB), 0, (hipStream_t)stream, p, q, w, n, similarity, out);
    return (int)hipGetLastError();
}
