// Mesh-to-mesh metrics (multiply_amd/metrics.py): the closest face of a triangle mesh to every query point, brute force, and
// the reduction of such a query to the numbers a reconstruction is judged by.  The indexed form of the query is
// k_index_closest (mesh_index.hip); both evaluate a face with tri_closest (mesh_prims.hpp), whose value does not depend on
// where it is inlined, and both select the lexicographic minimum of (d2, face id), so they return the same bits.
//   k_mesh_closest   a workgroup of 256 points walks the face list through LDS tiles of 512 faces, as k_mesh_sdist does: 18 KiB,
//                    every lane reads the same word of the tile at a time (a broadcast, no bank conflict), and a tile is
//                    read from memory once per four waves.  The lanes diverge inside tri_closest (seven regions); the loop
//                    around it is uniform.  Compute-bound: ~100 flops per point and face.
//   k_metric_reduce  ONE workgroup; per-thread partial sums in double over a strided walk, then wave shuffles and 16 LDS values
//                    summed in order by thread 0: a fixed order, bit-identical from call to call.  16 B per sample in,
//                    latency-bound at 10^5..10^6 samples.
// Entry points: include/multiply_hip.h mp_mesh_closest / mp_mesh_metric_reduce.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/multiply_hip.h"
#include "mesh_prims.hpp"

namespace {

constexpr int TB = 256, TILE = 512, RT = 1024, MAX_T = 8;

__global__ __launch_bounds__(TB) void k_mesh_closest(const float* __restrict__ pts, int n, const float* __restrict__ fv, int F,
                                                     float* __restrict__ d2_out, int* __restrict__ face_out,
                                                     float* __restrict__ q_out) {
    __shared__ float tri[TILE * 9];
    const int i = blockIdx.x * TB + threadIdx.x;
    float p[3] = {NAN, NAN, NAN};
    if (i < n) { p[0] = pts[3 * (size_t)i]; p[1] = pts[3 * (size_t)i + 1]; p[2] = pts[3 * (size_t)i + 2]; }
    const bool live = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);      // a non-finite point has no closest face
    float best = INFINITY, bq[3] = {NAN, NAN, NAN};
    int bid = -1;
    for (int f0 = 0; f0 < F; f0 += TILE) {
        const int nt = min(TILE, F - f0);
        __syncthreads();
        for (int k = threadIdx.x; k < nt * 9; k += TB) tri[k] = fv[(size_t)f0 * 9 + k];
        __syncthreads();
        if (live) {
            for (int t = 0; t < nt; ++t) {
                const float* a = tri + 9 * t;
                float q[3];
                const float d2 = tri_closest(p, a, a + 3, a + 6, q);
                const int id = f0 + t;
                // NaN (a zero-area face) and +inf fail both comparisons: best stays +inf with face -1
                if (d2 < best || (d2 == best && id < bid)) { best = d2; bid = id; bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2]; }
            }
        }
    }
    if (i >= n) return;
    d2_out[i] = best;
    if (face_out) face_out[i] = bid;
    if (q_out) { q_out[3 * (size_t)i] = bq[0]; q_out[3 * (size_t)i + 1] = bq[1]; q_out[3 * (size_t)i + 2] = bq[2]; }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sum of one double per thread, valid in thread 0: lanes by the xor butterfly, then the 16 waves in order
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();                       // the previous sum's reader is done with sh
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RT / 64; ++w) t += sh[w];
    return t;
}

__global__ __launch_bounds__(RT) void k_metric_reduce(const float* __restrict__ d2, const int* __restrict__ face,
                                                      const float* __restrict__ nrm, const float* __restrict__ fnrm, int n, int F,
                                                      const float* __restrict__ tau, int T, double* __restrict__ out) {
    __shared__ double sh[RT / 64];
    double s_d = 0.0, s_d2 = 0.0, s_nn = 0.0, s_abs = 0.0, mx = 0.0, cnt[MAX_T], valid = 0.0, left = 0.0;
    float th[MAX_T];
#pragma unroll
    for (int k = 0; k < MAX_T; ++k) { cnt[k] = 0.0; th[k] = k < T ? tau[k] : 0.f; }
    for (int i = threadIdx.x; i < n; i += RT) {
        const int f = face[i];
        if (f < 0 || f >= F) { left += 1.0; continue; }
        const float v2 = d2[i], d = sqrtf(v2);
        const float* a = nrm + 3 * (size_t)i;
        const float* b = fnrm + 3 * (size_t)f;
        const float c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        valid += 1.0;
        s_d += (double)d;
        s_d2 += (double)v2;
        s_nn += (double)c;
        s_abs += (double)fabsf(c);
        mx = fmax(mx, (double)d);
#pragma unroll
        for (int k = 0; k < MAX_T; ++k) cnt[k] += (k < T && d < th[k]) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 0; w < RT / 64; ++w) mx = fmax(mx, sh[w]);
    s_d = block_sum(s_d, sh);
    s_d2 = block_sum(s_d2, sh);
    s_nn = block_sum(s_nn, sh);
    s_abs = block_sum(s_abs, sh);
    valid = block_sum(valid, sh);
    left = block_sum(left, sh);
#pragma unroll
    for (int k = 0; k < MAX_T; ++k) cnt[k] = block_sum(cnt[k], sh);
    if (threadIdx.x == 0) {
        const double inv = valid > 0.0 ? 1.0 / valid : 0.0;
        out[0] = s_d * inv; out[1] = s_d2 * inv; out[2] = mx; out[3] = s_nn * inv; out[4] = s_abs * inv;
        out[5] = valid; out[6] = left;
#pragma unroll
        for (int k = 0; k < MAX_T; ++k)
            if (k < T) out[7 + k] = cnt[k];
    }
}

}  // namespace

extern "C" int mp_mesh_closest(const float* pts, int n, const float* face_verts, int n_faces, float* d2, int* face, float* q,
                               void* stream) {
    if (n < 0 || n_faces <= 0 || !face_verts || (n > 0 && (!pts || !d2))) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_mesh_closest, dim3((n + TB - 1) / TB), dim3(TB), 0, (hipStream_t)stream, pts, n, face_verts, n_faces, d2,
                       face, q);
    return (int)hipGetLastError();
}

extern "C" int mp_mesh_metric_reduce(const float* d2, const int* face, const float* normals, const float* face_normals, int n,
                                     int n_faces, const float* thresholds, int n_thresholds, double* out, void* stream) {
    if (n < 0 || n_faces <= 0 || n_thresholds < 0 || n_thresholds > MAX_T || !out || !face_normals) return -1;
    if (n_thresholds > 0 && !thresholds) return -1;
    if (n > 0 && (!d2 || !face || !normals)) return -1;
    hipLaunchKernelGGL(k_metric_reduce, dim3(1), dim3(RT), 0, (hipStream_t)stream, d2, face, normals, face_normals, n, n_faces,
                       thresholds, n_thresholds, out);
    return (int)hipGetLastError();
}
