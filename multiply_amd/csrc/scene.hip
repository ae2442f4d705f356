// Mask and bound kernels of the scene builder (multiply_amd/scene_build.py; the reference's `final` mode,
// preprocessing/preprocessing_multiple_trace.py:529-599, does these with cv2.dilate and numpy on the host, frame by frame).
// Entry points and layouts: include/multiply_hip.h.
//
//   mp_mask_dilate   binary dilation by a kh x kw box with an anchor, separable through LDS: one workgroup per DIL_TH x DIL_TW
//                    tile of the output loads the tile with its halo as 0 / 1 bytes, ORs kw neighbours along the rows of the halo,
//                    then kh along the columns.  Bytes outside the image are 0.
//   mp_mask_stats    count, bounding box and coordinate sums of the nonzero pixels: a workgroup reduces STAT_ROWS rows of one mask
//                    in registers / LDS and merges into the mask's seven 64-bit integers with integer atomics -- exact, and
//                    independent of the order.
//   mp_verts_bounds  per-frame min / max of the coordinates, or the largest distance from the origin after a per-frame shift: one
//                    workgroup per frame, wave reductions (common.hpp), no atomics.
#include <hip/hip_runtime.h>

#include "../../include/multiply_hip.h"
#include "common.hpp"

namespace {

constexpr int DIL_TH = 32, DIL_TW = 64, DIL_MAX_K = MP_DILATE_MAX_K, NT = 256;
constexpr int DIL_HR = DIL_TH + DIL_MAX_K - 1, DIL_HC = DIL_TW + DIL_MAX_K - 1;
constexpr int STAT_ROWS = 16;

__global__ __launch_bounds__(NT) void k_mask_dilate(const unsigned char* __restrict__ in, int H, int W, int kh, int kw, int ay,
                                                    int ax, unsigned char* __restrict__ out) {
    __shared__ unsigned char a[DIL_HR * DIL_HC];    // the tile with its halo, 0 / 1
    __shared__ unsigned char b[DIL_HR * DIL_TW];    // after the row pass
    const int t = threadIdx.x;
    const int r0 = blockIdx.y * DIL_TH, c0 = blockIdx.x * DIL_TW;
    const size_t img = (size_t)blockIdx.z * H * W;
    const int hr = DIL_TH + kh - 1, hc = DIL_TW + kw - 1;
    for (int i = t; i < hr * hc; i += NT) {
        const int r = r0 - ay + i / hc, c = c0 - ax + i % hc;
        a[i] = (r >= 0 && r < H && c >= 0 && c < W) ? (in[img + (size_t)r * W + c] != 0) : 0;
    }
    __syncthreads();
    for (int i = t; i < hr * DIL_TW; i += NT) {
        const unsigned char* p = a + (i / DIL_TW) * hc + i % DIL_TW;
        unsigned char v = 0;
        for (int k = 0; k < kw; ++k) v |= p[k];
        b[i] = v;
    }
    __syncthreads();
    for (int i = t; i < DIL_TH * DIL_TW; i += NT) {
        const int r = i / DIL_TW, c = i % DIL_TW;
        if (r0 + r >= H || c0 + c >= W) continue;
        unsigned char v = 0;
        for (int k = 0; k < kh; ++k) v |= b[(r + k) * DIL_TW + c];
        out[img + (size_t)(r0 + r) * W + c0 + c] = v ? 255 : 0;
    }
}

__global__ void k_stats_init(long long* __restrict__ stats, int N, int H, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * 7) return;
    const int k = i % 7;
    stats[i] = k == 1 ? H : (k == 3 ? W : ((k == 2 || k == 4) ? -1 : 0));
}

__device__ __forceinline__ long long wsum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wmin_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wmax_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(NT) void k_mask_stats(const unsigned char* __restrict__ mask, int H, int W,
                                                   long long* __restrict__ stats) {
    __shared__ long long sh[4][7];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned char* m = mask + (size_t)blockIdx.y * H * W;
    const int rb = blockIdx.x * STAT_ROWS, re = min(H, rb + STAT_ROWS);
    long long cnt = 0, sr = 0, sc = 0;
    int rmin = H, rmax = -1, cmin = W, cmax = -1;
    for (int r = rb; r < re; ++r) {
        const unsigned char* row = m + (size_t)r * W;
        int k = 0;
        long long s = 0;
        for (int c = t; c < W; c += NT)
            if (row[c]) {
                ++k;
                s += c;
                cmin = min(cmin, c);
                cmax = max(cmax, c);
            }
        if (k) {
            cnt += k;
            sr += (long long)k * r;
            sc += s;
            rmin = min(rmin, r);
            rmax = max(rmax, r);
        }
    }
    cnt = wsum_ll(cnt); sr = wsum_ll(sr); sc = wsum_ll(sc);
    rmin = wmin_i(rmin); rmax = wmax_i(rmax); cmin = wmin_i(cmin); cmax = wmax_i(cmax);
    if (lane == 0) {
        sh[wave][0] = cnt; sh[wave][1] = rmin; sh[wave][2] = rmax; sh[wave][3] = cmin; sh[wave][4] = cmax;
        sh[wave][5] = sr; sh[wave][6] = sc;
    }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < 4; ++w) {
        sh[0][0] += sh[w][0]; sh[0][5] += sh[w][5]; sh[0][6] += sh[w][6];
        sh[0][1] = min(sh[0][1], sh[w][1]); sh[0][2] = max(sh[0][2], sh[w][2]);
        sh[0][3] = min(sh[0][3], sh[w][3]); sh[0][4] = max(sh[0][4], sh[w][4]);
    }
    if (sh[0][0] == 0) return;
    long long* o = stats + (size_t)blockIdx.y * 7;
    atomicAdd((unsigned long long*)o, (unsigned long long)sh[0][0]);
    atomicMin(o + 1, sh[0][1]);
    atomicMax(o + 2, sh[0][2]);
    atomicMin(o + 3, sh[0][3]);
    atomicMax(o + 4, sh[0][4]);
    atomicAdd((unsigned long long*)(o + 5), (unsigned long long)sh[0][5]);
    atomicAdd((unsigned long long*)(o + 6), (unsigned long long)sh[0][6]);
}

// shift == NULL: out [F][6] = min xyz, max xyz;  else out [F] = max |v + shift_f|
__global__ __launch_bounds__(NT) void k_verts_bounds(const float* __restrict__ verts, int n, const float* __restrict__ shift,
                                                     float* __restrict__ out) {
    __shared__ float sh[4][6];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, f = blockIdx.x;
    const float* v = verts + (size_t)f * n * 3;
    if (shift) {
        const float sx = shift[3 * f], sy = shift[3 * f + 1], sz = shift[3 * f + 2];
        float d2 = 0.f;
        for (int i = t; i < n; i += NT) {
            const float x = v[3 * i] + sx, y = v[3 * i + 1] + sy, z = v[3 * i + 2] + sz;
            d2 = fmaxf(d2, x * x + y * y + z * z);
        }
        d2 = mp::wmax(d2);
        if (lane == 0) sh[wave][0] = d2;
        __syncthreads();
        if (t == 0) out[f] = sqrtf(fmaxf(fmaxf(sh[0][0], sh[1][0]), fmaxf(sh[2][0], sh[3][0])));
        return;
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < n; i += NT)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = v[3 * i + k];
            lo[k] = fminf(lo[k], x);
            hi[k] = fmaxf(hi[k], x);
        }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = mp::wmin(lo[k]);
        hi[k] = mp::wmax(hi[k]);
        if (lane == 0) { sh[wave][k] = lo[k]; sh[wave][3 + k] = hi[k]; }
    }
    __syncthreads();
    if (t < 6) {
        const float a = sh[0][t], b = sh[1][t], c = sh[2][t], d = sh[3][t];
        out[6 * f + t] = t < 3 ? fminf(fminf(a, b), fminf(c, d)) : fmaxf(fmaxf(a, b), fmaxf(c, d));
    }
}

}  // namespace

extern "C" int mp_mask_dilate(const unsigned char* in, int N, int H, int W, int kh, int kw, int ay, int ax, unsigned char* out,
                              void* stream) {
    if (N < 0 || H <= 0 || W <= 0) return -1;
    if (kh < 1 || kw < 1 || kh > DIL_MAX_K || kw > DIL_MAX_K || ay < 0 || ay >= kh || ax < 0 || ax >= kw) return -2;
    if (N == 0) return 0;
    if (!in || !out || in == out || N > 65535) return -1;
    const dim3 grid((W + DIL_TW - 1) / DIL_TW, (H + DIL_TH - 1) / DIL_TH, N);
    if (grid.y > 65535) return -1;
    hipLaunchKernelGGL(k_mask_dilate, grid, dim3(NT), 0, (hipStream_t)stream, in, H, W, kh, kw, ay, ax, out);
    return (int)hipGetLastError();
}

extern "C" int mp_mask_stats(const unsigned char* mask, int N, int H, int W, long long* stats, void* stream) {
    if (N < 0 || H <= 0 || W <= 0) return -1;
    if (N == 0) return 0;
    if (!mask || !stats || N > 65535) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_stats_init, dim3((N * 7 + 255) / 256), dim3(256), 0, st, stats, N, H, W);
    hipLaunchKernelGGL(k_mask_stats, dim3((H + STAT_ROWS - 1) / STAT_ROWS, N), dim3(NT), 0, st, mask, H, W, stats);
    return (int)hipGetLastError();
}

extern "C" int mp_verts_bounds(const float* verts, int F, int n, const float* shift, float* out, void* stream) {
    if (F < 0 || n < 1) return -1;
    if (F == 0) return 0;
    if (!verts || !out) return -1;
    hipLaunchKernelGGL(k_verts_bounds, dim3(F), dim3(NT), 0, (hipStream_t)stream, verts, n, shift, out);
    return (int)hipGetLastError();
}
