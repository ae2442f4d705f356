// Mesh simplification by vertex clustering with quadric-optimal representatives (multiply_amd/simplify.py; contracts:
// include/multiply_hip.h).  The host sorts between the launches; what reads a coordinate is here.
//   k_simplify_keys      one thread per vertex: the cell key, fp32 subtraction and multiplication rounded to nearest.
//   k_simplify_count     one thread per face: are the three corners' keys pairwise different (the bisection's count pass).
//   k_simplify_faces     one thread per face: corners -> cell ids, the live flag, the unordered triple as a two-word sort key.
//   k_simplify_first     one thread per sorted position: the first face of each run of equal triples is kept.
//   k_simplify_quadrics  MP_SIMPLIFY_LANES lanes per cell.  A cell's lists (its (corner, face) pairs, its own vertices) are
//                        sorted segments; lane l walks entries l, l + LANES, ... in order with 12 double accumulators, the lanes
//                        meet in the xor butterfly, lane 0 solves (quadric_solve.hpp) and stores.  The order of every sum is a
//                        function of the segment alone: no atomics, the same bits on every run.  Why 16 lanes: the segments of a
//                        useful reduction hold dozens to hundreds of entries, each a dependent gather (order -> face -> three
//                        vertices); one lane per cell leaves 63 lanes of a wave waiting on the longest cell's chain, a whole wave
//                        per cell idles most lanes on a short segment and spends six shuffle rounds on 12 doubles.  Measured
//                        times: profiles/simplify.txt.
//   k_simplify_attr_mean one thread per (cell, column): consecutive threads read consecutive columns of one row.
// No fused multiply-adds in this file: a face with two equal edge vectors must give n = 0 EXACTLY, as in the float64 reference
// (trace(A) == 0 selects the mean), and the keys must be the reference's bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/multiply_hip.h"
#include "quadric_solve.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int TB = 256, G = MP_SIMPLIFY_LANES;
constexpr long long IDX_MASK = MP_SIMPLIFY_MAX_INDEX;

__device__ __forceinline__ long long cell_index(float v, float lo, float inv_h) {
    const float q = floorf(__fmul_rn(__fsub_rn(v, lo), inv_h));
    return q > 0.0f ? (q < (float)MP_SIMPLIFY_MAX_INDEX ? (long long)q : IDX_MASK) : 0;       // (a NaN gives 0)
}

__global__ __launch_bounds__(TB) void k_simplify_keys(const float* __restrict__ verts, int n, float lx, float ly, float lz,
                                                      float inv_h, long long* __restrict__ key) {
    const int v = blockIdx.x * TB + threadIdx.x;
    if (v >= n) return;
    const float* p = verts + 3 * (size_t)v;
    key[v] = (cell_index(p[0], lx, inv_h) << (2 * MP_SIMPLIFY_BITS)) | (cell_index(p[1], ly, inv_h) << MP_SIMPLIFY_BITS) |
             cell_index(p[2], lz, inv_h);
}

__global__ __launch_bounds__(TB) void k_simplify_count(const int* __restrict__ faces, int n_faces, const long long* __restrict__ key,
                                                       int n_verts, unsigned char* __restrict__ live) {
    const int f = blockIdx.x * TB + threadIdx.x;
    if (f >= n_faces) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    bool ok = (unsigned)a < (unsigned)n_verts && (unsigned)b < (unsigned)n_verts && (unsigned)c < (unsigned)n_verts;
    if (ok) {
        const long long ka = key[a], kb = key[b], kc = key[c];
        ok = ka != kb && kb != kc && ka != kc;
    }
    live[f] = ok ? 1 : 0;
}

__global__ __launch_bounds__(TB) void k_simplify_faces(const int* __restrict__ faces, int n_faces, const int* __restrict__ cell,
                                                       int n_verts, int* __restrict__ tri, long long* __restrict__ key_lo,
                                                       int* __restrict__ key_hi, unsigned char* __restrict__ live) {
    const int f = blockIdx.x * TB + threadIdx.x;
    if (f >= n_faces) return;
    int id[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * (size_t)f + k];
        const bool in = (unsigned)v < (unsigned)n_verts;
        id[k] = in ? cell[v] : 0;
        ok = ok && in;
        tri[3 * (size_t)f + k] = id[k];
    }
    ok = ok && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    const int lo = min(id[0], min(id[1], id[2])), hi = max(id[0], max(id[1], id[2]));
    const int mid = id[0] ^ id[1] ^ id[2] ^ lo ^ hi;                 // the three are distinct where this is used
    live[f] = ok ? 1 : 0;
    key_lo[f] = ok ? (((long long)lo << 32) | (long long)mid) : 0x7fffffffffffffffLL;
    key_hi[f] = ok ? hi : 0x7fffffff;
}

__global__ __launch_bounds__(TB) void k_simplify_first(const long long* __restrict__ order, int n_faces,
                                                       const long long* __restrict__ key_lo, const int* __restrict__ key_hi,
                                                       const unsigned char* __restrict__ live, unsigned char* __restrict__ keep) {
    const int s = blockIdx.x * TB + threadIdx.x;
    if (s >= n_faces) return;
    const long long f = order[s];
    if (f < 0 || f >= n_faces) return;
    bool first = live[f] != 0;
    if (first && s > 0) {
        const long long g = order[s - 1];
        if (g >= 0 && g < n_faces) first = key_lo[g] != key_lo[f] || key_hi[g] != key_hi[f];
    }
    keep[f] = first ? 1 : 0;
}

__global__ __launch_bounds__(TB) void k_simplify_quadrics(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                          int n_faces, const long long* __restrict__ keys, int n_cells,
                                                          const long long* __restrict__ pair_order,
                                                          const long long* __restrict__ pair_start,
                                                          const long long* __restrict__ vert_order,
                                                          const long long* __restrict__ vert_start, float lx, float ly, float lz,
                                                          float h, double lam, float* __restrict__ pos) {
    const int lane = threadIdx.x % G;
    const long long c = (long long)blockIdx.x * (TB / G) + threadIdx.x / G;
    if (c >= n_cells) return;                                        // all G lanes of the cell at once
    const long long key = keys[c];
    const double h64 = (double)h;
    const double ctr[3] = {(double)lx + ((double)(key >> (2 * MP_SIMPLIFY_BITS)) + 0.5) * h64,
                           (double)ly + ((double)((key >> MP_SIMPLIFY_BITS) & IDX_MASK) + 0.5) * h64,
                           (double)lz + ((double)(key & IDX_MASK) + 0.5) * h64};
    double acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0.0;
    const long long p_end = pair_start[c + 1], n_pairs = 3LL * n_faces;
    for (long long s = pair_start[c] + lane; s < p_end; s += G) {
        if (s < 0 || s >= n_pairs) break;
        const long long p = pair_order[s];
        if (p < 0 || p >= n_pairs) continue;
        const size_t f = (size_t)(p / 3);
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if ((unsigned)i0 >= (unsigned)n_verts || (unsigned)i1 >= (unsigned)n_verts || (unsigned)i2 >= (unsigned)n_verts) continue;
        double p0[3], a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            p0[k] = (double)verts[3 * (size_t)i0 + k];
            a[k] = (double)verts[3 * (size_t)i1 + k] - p0[k];
            b[k] = (double)verts[3 * (size_t)i2 + k] - p0[k];
        }
        const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double d[3] = {p0[0] - ctr[0], p0[1] - ctr[1], p0[2] - ctr[2]};
        const double nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
        acc[0] += n[0] * n[0]; acc[1] += n[0] * n[1]; acc[2] += n[0] * n[2];
        acc[3] += n[1] * n[1]; acc[4] += n[1] * n[2]; acc[5] += n[2] * n[2];
        acc[6] += n[0] * nd; acc[7] += n[1] * nd; acc[8] += n[2] * nd;
    }
    const long long v_begin = vert_start[c], v_end = vert_start[c + 1];
    for (long long s = v_begin + lane; s < v_end; s += G) {
        if (s < 0 || s >= n_verts) break;
        const long long v = vert_order[s];
        if (v < 0 || v >= n_verts) continue;
        for (int k = 0; k < 3; ++k) acc[9 + k] += (double)verts[3 * (size_t)v + k] - ctr[k];
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1)
#pragma unroll
        for (int j = 0; j < 12; ++j) acc[j] += __shfl_xor(acc[j], o, G);
    if (lane != 0) return;
    const double count = (double)(v_end - v_begin);
    const double mean[3] = {acc[9] / fmax(count, 1.0), acc[10] / fmax(count, 1.0), acc[11] / fmax(count, 1.0)};
    double x[3];
    quadric_point(acc, acc + 6, mean, lam, 0.5 * h64, x, nullptr);
    for (int k = 0; k < 3; ++k) pos[3 * (size_t)c + k] = (float)(ctr[k] + x[k]);
}

__global__ __launch_bounds__(TB) void k_simplify_attr_mean(const float* __restrict__ attrs, int n_verts, int K,
                                                           const long long* __restrict__ vert_order,
                                                           const long long* __restrict__ vert_start, long long total,
                                                           float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * TB + threadIdx.x;
    if (t >= total) return;
    const long long c = t / K;
    const int k = (int)(t - c * K);
    const long long v_begin = vert_start[c], v_end = vert_start[c + 1];
    double sum = 0.0;
    for (long long s = v_begin; s < v_end; ++s) {
        if (s < 0 || s >= n_verts) break;
        const long long v = vert_order[s];
        if (v < 0 || v >= n_verts) continue;
        sum += (double)attrs[(size_t)v * K + k];
    }
    out[t] = (float)(sum / fmax((double)(v_end - v_begin), 1.0));
}

inline int blocks(long long n) { return (int)((n + TB - 1) / TB); }
}  // namespace

extern "C" int mp_simplify_keys(const float* verts, int n_verts, float lo_x, float lo_y, float lo_z, float inv_h, long long* key,
                                void* stream) {
    if (n_verts < 0 || !(inv_h > 0.0f) || !isfinite(inv_h) || (n_verts > 0 && (!verts || !key))) return -1;
    if (n_verts == 0) return 0;
    hipLaunchKernelGGL(k_simplify_keys, dim3(blocks(n_verts)), dim3(TB), 0, (hipStream_t)stream, verts, n_verts, lo_x, lo_y, lo_z,
                       inv_h, key);
    return (int)hipGetLastError();
}

extern "C" int mp_simplify_count(const int* faces, int n_faces, const long long* key, int n_verts, unsigned char* live, void* stream) {
    if (n_faces < 0 || n_verts < 0 || (n_faces > 0 && (!faces || !live || (n_verts > 0 && !key)))) return -1;
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(k_simplify_count, dim3(blocks(n_faces)), dim3(TB), 0, (hipStream_t)stream, faces, n_faces, key, n_verts, live);
    return (int)hipGetLastError();
}

extern "C" int mp_simplify_faces(const int* faces, int n_faces, const int* cell, int n_verts, int* tri, long long* key_lo, int* key_hi,
                                 unsigned char* live, void* stream) {
    if (n_faces < 0 || n_verts < 0 || (n_faces > 0 && (!faces || !tri || !key_lo || !key_hi || !live || (n_verts > 0 && !cell))))
        return -1;
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(k_simplify_faces, dim3(blocks(n_faces)), dim3(TB), 0, (hipStream_t)stream, faces, n_faces, cell, n_verts, tri,
                       key_lo, key_hi, live);
    return (int)hipGetLastError();
}

extern "C" int mp_simplify_first(const long long* order, int n_faces, const long long* key_lo, const int* key_hi,
                                 const unsigned char* live, unsigned char* keep, void* stream) {
    if (n_faces < 0 || (n_faces > 0 && (!order || !key_lo || !key_hi || !live || !keep))) return -1;
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(k_simplify_first, dim3(blocks(n_faces)), dim3(TB), 0, (hipStream_t)stream, order, n_faces, key_lo, key_hi, live,
                       keep);
    return (int)hipGetLastError();
}

extern "C" int mp_simplify_quadrics(const float* verts, int n_verts, const int* faces, int n_faces, const long long* keys, int n_cells,
                                    const long long* pair_order, const long long* pair_start, const long long* vert_order,
                                    const long long* vert_start, float lo_x, float lo_y, float lo_z, float h, double lam, float* pos,
                                    void* stream) {
    if (n_verts < 0 || n_faces < 0 || n_cells < 0 || 3LL * n_faces >= (1LL << 31) || !(h > 0.0f) || !isfinite(h) || !(lam > 0.0) ||
        !isfinite(lam))
        return -1;
    if (n_cells > 0 && (!verts || !keys || !pair_start || !vert_order || !vert_start || !pos || n_verts == 0 ||
                        (n_faces > 0 && (!faces || !pair_order))))
        return -1;
    if (n_cells == 0) return 0;
    hipLaunchKernelGGL(k_simplify_quadrics, dim3((n_cells + TB / G - 1) / (TB / G)), dim3(TB), 0, (hipStream_t)stream, verts, n_verts,
                       faces, n_faces, keys, n_cells, pair_order, pair_start, vert_order, vert_start, lo_x, lo_y, lo_z, h, lam, pos);
    return (int)hipGetLastError();
}

extern "C" int mp_simplify_attr_mean(const float* attrs, int n_verts, int K, const long long* vert_order, const long long* vert_start,
                                     int n_cells, float* out, void* stream) {
    const long long total = (long long)n_cells * K;
    if (n_verts < 0 || K < 0 || n_cells < 0 || total >= (1LL << 38)) return -1;
    if (total > 0 && (!attrs || !vert_order || !vert_start || !out || n_verts == 0)) return -1;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_simplify_attr_mean, dim3(blocks(total)), dim3(TB), 0, (hipStream_t)stream, attrs, n_verts, K, vert_order,
                       vert_start, total, out);
    return (int)hipGetLastError();
}
