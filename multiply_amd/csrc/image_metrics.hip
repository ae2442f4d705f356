// Image-space metrics (multiply_amd/image_metrics.py): the per-frame sums PSNR and SSIM are made of.
//   k_image_ssim    one workgroup of 256 threads per T x T tile of the SSIM map (T = MP_SSIM_TILE = 32) of one frame, the channels
//                   one after the other.  Per channel: the tile and its 10-pixel halo of both images go to LDS as floats
//                   ((T+10)^2 each; rows are W*C contiguous floats with the taps at stride C, so nothing is transposed on the
//                   host), then the horizontal pass over the five quantities a, b, a^2, b^2, ab ((T+10) x T doubles each), the
//                   vertical pass and the SSIM expression.  71 KiB of LDS: two workgroups per CU.  Everything after the load is
//                   in double: ~110 multiply-adds per map value, the fp64 vector rate bounds the kernel, not memory.
//                   Cancellation: the moments are taken about a PIVOT (the tile's first pixel of each image), variances and the
//                   covariance do not depend on it, and on the flat frames a renderer produces the raw moments about it are
//                   tiny: E[x^2] - mu^2 then loses nothing (two constant images give variance 0 exactly).
//                   Symmetry: a and b go through the same operations, the expression has contraction off and is written so
//                   that swapping a and b swaps commutative operands only: ssim(a, b) and ssim(b, a) have equal bits, and
//                   ssim(a, a) is exactly 1 wherever it is defined.
//                   A non-finite value of a or b enters the sums as the pivot and raises a count that travels through both
//                   passes: a window with a non-zero count is left out (map value NaN).
//   k_image_sqerr   one workgroup per 4096 consecutive values of a frame (coalesced scalar loads: a frame's first value need not
//                   be 16-byte aligned), (a - b)^2 in double.  Memory-bound: 8 B per value.
//   k_image_finish  one workgroup per frame adds that frame's partials [5] in a fixed order.
// No atomics: every number is bit-identical from call to call.  Entry points: include/multiply_hip.h mp_image_*.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "../../include/multiply_hip.h"

namespace {

constexpr int T = MP_SSIM_TILE, WIN = 11, HALO = WIN - 1, R = T + HALO, TB = 256, NQ = 5, NOUT = 5, SQ_CHUNK = 4096;

struct Taps { double g[WIN]; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the workgroup's sums of NOUT doubles per thread -> dst[NOUT] (thread 0): lanes by the xor butterfly, then the waves in order
__device__ __forceinline__ void block_sums(const double* v, double (*sh)[NOUT], double* dst) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
        const double s = wave_sum(v[j]);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][j] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) {
            double t = 0.0;
            for (int w = 0; w < TB / 64; ++w) t += sh[w][j];
            dst[j] = t;
        }
    }
}

// SSIM of one window from its moments about the pivots (pa, pb): m = E[x - p], e = E[(x - p)(y - q)].  Every operation is rounded
// on its own, and a <-> b exchanges the operands of commutative operations only.
__device__ __forceinline__ double ssim_value(double pa, double pb, double ma, double mb, double eaa, double ebb, double eab,
                                             double C1, double C2) {
#pragma clang fp contract(off)
    const double mua = pa + ma, mub = pb + mb;
    const double va = eaa - ma * ma, vb = ebb - mb * mb, cab = eab - ma * mb;
    const double num = (2.0 * (mua * mub) + C1) * (2.0 * cab + C2);
    const double den = ((mua * mua + mub * mub) + C1) * ((va + vb) + C2);
    return num / den;
}

__global__ __launch_bounds__(TB) void k_image_ssim(const float* __restrict__ a, const float* __restrict__ b,
                                                   const unsigned char* __restrict__ mask, int H, int W, int C, double C1,
                                                   double C2, Taps taps, int tiles_x, int tiles_per_frame,
                                                   double* __restrict__ partial, float* __restrict__ map) {
    __shared__ float sa[R * R], sb[R * R];
    __shared__ double hb[NQ][R * T];
    __shared__ unsigned char sbad[R * R], hbad[R * T];
    __shared__ double red[TB / 64][NOUT];
    const int n = blockIdx.x / tiles_per_frame, tile = blockIdx.x % tiles_per_frame;
    const int y0 = (tile / tiles_x) * T, x0 = (tile % tiles_x) * T, OH = H - HALO, OW = W - HALO;
    const size_t pix0 = (size_t)n * H * W;
    const float* fa = a + pix0 * C;
    const float* fb = b + pix0 * C;
    double acc[NOUT] = {0.0, 0.0, 0.0, 0.0, 0.0};       // sum, count, masked sum, masked count, left out
    for (int c = 0; c < C; ++c) {
        // (y0, x0) is inside the image: the tile holds at least one window
        float pa = fa[((size_t)y0 * W + x0) * C + c], pb = fb[((size_t)y0 * W + x0) * C + c];
        if (!isfinite(pa)) pa = 0.f;
        if (!isfinite(pb)) pb = 0.f;
        // no barrier here: the previous channel's horizontal pass (the last reader of sa / sb / sbad) ended at a barrier, and the
        // barrier after this loop keeps the next horizontal pass off hb / hbad until the previous vertical pass is done with them
        for (int i = threadIdx.x; i < R * R; i += TB) {
            const int y = y0 + i / R, x = x0 + i % R;
            float va = pa, vb = pb;
            unsigned char bad = 0;
            if (y < H && x < W) {                        // beyond the image: pivots, which only windows that do not exist read
                const size_t e = ((size_t)y * W + x) * C + c;
                va = fa[e];
                vb = fb[e];
                if (!(isfinite(va) && isfinite(vb))) { bad = 1; va = pa; vb = pb; }
            }
            sa[i] = va; sb[i] = vb; sbad[i] = bad;
        }
        __syncthreads();
        const double da0 = (double)pa, db0 = (double)pb;
        for (int i = threadIdx.x; i < R * T; i += TB) {
            const int r = i / T, x = i % T;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
            int nb = 0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double w = taps.g[k], da = (double)sa[r * R + x + k] - da0, db = (double)sb[r * R + x + k] - db0;
                h0 += w * da; h1 += w * db; h2 += w * (da * da); h3 += w * (db * db); h4 += w * (da * db);
                nb += sbad[r * R + x + k];
            }
            hb[0][i] = h0; hb[1][i] = h1; hb[2][i] = h2; hb[3][i] = h3; hb[4][i] = h4;
            hbad[i] = (unsigned char)nb;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < T * T; i += TB) {
            const int y = i / T, x = i % T, oy = y0 + y, ox = x0 + x;
            if (oy >= OH || ox >= OW) continue;
            double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
            int nb = 0;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const double w = taps.g[k];
                const int j = (y + k) * T + x;
                v0 += w * hb[0][j]; v1 += w * hb[1][j]; v2 += w * hb[2][j]; v3 += w * hb[3][j]; v4 += w * hb[4][j];
                nb += hbad[j];
            }
            float stored = NAN;
            if (nb) {
                acc[4] += 1.0;
            } else {
                const double s = ssim_value(da0, db0, v0, v1, v2, v3, v4, C1, C2);
                acc[0] += s; acc[1] += 1.0;
                if (!mask || mask[pix0 + (size_t)(oy + HALO / 2) * W + (ox + HALO / 2)]) { acc[2] += s; acc[3] += 1.0; }
                stored = (float)s;
            }
            if (map) map[(((size_t)n * OH + oy) * OW + ox) * C + c] = stored;
        }
    }
    block_sums(acc, red, partial + (size_t)blockIdx.x * NOUT);
}

__global__ __launch_bounds__(TB) void k_image_sqerr(const float* __restrict__ a, const float* __restrict__ b,
                                                    const unsigned char* __restrict__ mask, unsigned E, unsigned C,
                                                    int blocks_per_frame, double* __restrict__ partial) {
    __shared__ double red[TB / 64][NOUT];
    const int n = blockIdx.x / blocks_per_frame, blk = blockIdx.x % blocks_per_frame;
    const float* fa = a + (size_t)n * E;
    const float* fb = b + (size_t)n * E;
    const unsigned char* fm = mask ? mask + (size_t)n * (E / C) : nullptr;
    double acc[NOUT] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int i = 0; i < SQ_CHUNK / TB; ++i) {
        const unsigned long long e64 = (unsigned long long)blk * SQ_CHUNK + (unsigned)(i * TB) + threadIdx.x;
        if (e64 >= E) break;
        const unsigned e = (unsigned)e64;
        const float va = fa[e], vb = fb[e];
        if (isfinite(va) && isfinite(vb)) {
            const double d = (double)va - (double)vb, d2 = d * d;
            acc[0] += d2; acc[1] += 1.0;
            if (!fm || fm[e / C]) { acc[2] += d2; acc[3] += 1.0; }
        } else {
            acc[4] += 1.0;
        }
    }
    block_sums(acc, red, partial + (size_t)blockIdx.x * NOUT);
}

__global__ __launch_bounds__(TB) void k_image_finish(const double* __restrict__ partial, int per_frame, double* __restrict__ out) {
    __shared__ double red[TB / 64][NOUT];
    const double* p = partial + (size_t)blockIdx.x * per_frame * NOUT;
    double acc[NOUT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < per_frame; i += TB)
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] += p[(size_t)i * NOUT + j];
    block_sums(acc, red, out + (size_t)blockIdx.x * NOUT);
}

inline long long ssim_tiles(int H, int W, int* tiles_x) {
    const int tx = (W - HALO + T - 1) / T, ty = (H - HALO + T - 1) / T;
    if (tiles_x) *tiles_x = tx;
    return (long long)tx * ty;
}

inline long long sqerr_blocks(int H, int W, int C) { return ((long long)H * W * C + SQ_CHUNK - 1) / SQ_CHUNK; }

}  // namespace

extern "C" int mp_image_work_bytes(int N, int H, int W, int C) {
    if (N < 0 || H < 1 || W < 1 || (C != 1 && C != 3)) return -1;
    long long per = sqerr_blocks(H, W, C);
    if (H >= WIN && W >= WIN) per = per > ssim_tiles(H, W, nullptr) ? per : ssim_tiles(H, W, nullptr);
    const long long bytes = per * N * NOUT * (long long)sizeof(double);
    return bytes > INT_MAX ? -1 : (int)bytes;
}

extern "C" int mp_image_ssim(const float* a, const float* b, const unsigned char* mask, int N, int H, int W, int C, float data_range,
                             void* work, double* out, float* map, void* stream) {
    if (N < 0 || H < WIN || W < WIN || (C != 1 && C != 3) || !(data_range > 0.f) || !isfinite(data_range)) return -1;
    if (N == 0) return 0;
    if (!a || !b || !work || !out) return -1;
    int tiles_x;
    const long long per = ssim_tiles(H, W, &tiles_x);
    if (per * N > INT_MAX) return -1;
    Taps taps;
    double sum = 0.0;
    for (int k = 0; k < WIN; ++k) { taps.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)); sum += taps.g[k]; }
    for (int k = 0; k < WIN; ++k) taps.g[k] /= sum;
    const double L = (double)data_range, C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    hipLaunchKernelGGL(k_image_ssim, dim3((unsigned)(per * N)), dim3(TB), 0, (hipStream_t)stream, a, b, mask, H, W, C, C1, C2, taps,
                       tiles_x, (int)per, (double*)work, map);
    hipLaunchKernelGGL(k_image_finish, dim3(N), dim3(TB), 0, (hipStream_t)stream, (const double*)work, (int)per, out);
    return (int)hipGetLastError();
}

extern "C" int mp_image_sqerr(const float* a, const float* b, const unsigned char* mask, int N, int H, int W, int C, void* work,
                              double* out, void* stream) {
    if (N < 0 || H < 1 || W < 1 || (C != 1 && C != 3) || (long long)H * W * C > INT_MAX) return -1;
    if (N == 0) return 0;
    if (!a || !b || !work || !out) return -1;
    const long long per = sqerr_blocks(H, W, C);
    if (per * N > INT_MAX) return -1;
    hipLaunchKernelGGL(k_image_sqerr, dim3((unsigned)(per * N)), dim3(TB), 0, (hipStream_t)stream, a, b, mask,
                       (unsigned)((long long)H * W * C), (unsigned)C, (int)per, (double*)work);
    hipLaunchKernelGGL(k_image_finish, dim3(N), dim3(TB), 0, (hipStream_t)stream, (const double*)work, (int)per, out);
    return (int)hipGetLastError();
}
