// Mesh-free interpenetration term on the persons' SDF fields (train.py Interpenetration): person p's posed SMPL vertices are probe
// points, warped into partner q's canonical space by q's exact nearest posed vertex and penalised by q's signed distance where
// it is negative.  Three entry points, each ONE call for all ordered pairs (p, q), p != q, pair index p * P + q:
//   mp_pen_probe        the cross-person nearest-vertex search capped at the outlier radius, x_c, and the compact ascending list
//   mp_pen_loss         L_pq = sum of s^2 over {s < 0}, the active counts, the adjoint's seed 2 s [s < 0]
//   mp_pen_scatter_bwd  d x = I_nn^T d x_c gathered onto the probing person's drawn vertices
// Everything is deterministic: no returning atomic decides an order, no float atomic forms a sum.
// Entry points: include/multiply_hip.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "knn_search.hpp"
#include "ray_merge.hpp"      // mp::MAX_P: the person limit of a call

namespace {

constexpr int NC = MP_KNN_NC, CL = MP_KNN_CLUSTER;
constexpr int PROBE_THREADS = 512;
constexpr int PROBE_LDS = NC * CL * 16 + NC * 16 + 32;      // q's vertices, their cluster spheres, the box of all vertices
constexpr int COMPACT_THREADS = 1024, TB = 256;

// grid (blocks per pair, P * P).  A block holds q's posed vertex structure in LDS and walks slabs of 64 probe points of p.
__global__ __launch_bounds__(PROBE_THREADS) void k_pen_probe(const float* const* __restrict__ pts_tab,
                                                             const float* const* __restrict__ vs_tab,
                                                             const float* const* __restrict__ cb_tab,
                                                             const float* const* __restrict__ bt_tab, int P, int n,
                                                             unsigned char* __restrict__ probed, int* __restrict__ nn,
                                                             float* __restrict__ xc) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int pair = blockIdx.y, p = pair / P, q = pair - p * P;
    if (p == q) return;
    float4* vs = (float4*)smem;
    float4* cb = vs + NC * CL;
    float* box = (float*)(cb + NC);      // [6] conservative bounds of q's vertices, grown by the outlier radius
    load_knn_lds(vs, cb, vs_tab[q], cb_tab[q]);
    __syncthreads();
    if (threadIdx.x < 64) {
        float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int c = threadIdx.x; c < NC; c += 64) {
            const float4 b = cb[c];
            lo[0] = fminf(lo[0], b.x - b.w); lo[1] = fminf(lo[1], b.y - b.w); lo[2] = fminf(lo[2], b.z - b.w);
            hi[0] = fmaxf(hi[0], b.x + b.w); hi[1] = fmaxf(hi[1], b.y + b.w); hi[2] = fmaxf(hi[2], b.z + b.w);
        }
        for (int a = 0; a < 3; ++a) { lo[a] = mp::wmin(lo[a]); hi[a] = mp::wmax(hi[a]); }
        if (threadIdx.x == 0) for (int a = 0; a < 3; ++a) { box[a] = lo[a] - 0.1005f; box[3 + a] = hi[a] + 0.1005f; }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const float* __restrict__ pts = pts_tab[p];
    const float4* __restrict__ bt = (const float4*)bt_tab[q];
    const size_t row0 = (size_t)pair * n;
    const float cap2 = 0.0101f;      // k_warp_inverse's eval cap: only neighbours within the 0.1 outlier radius matter
    const int n_slab = (n + 63) / 64;
    for (int slab = blockIdx.x * nw + wave; slab < n_slab; slab += gridDim.x * nw) {
        const int i = slab * 64 + lane;
        const bool on = i < n;
        float x = 0.f, y = 0.f, z = 0.f;
        if (on) { x = pts[3 * (size_t)i]; y = pts[3 * (size_t)i + 1]; z = pts[3 * (size_t)i + 2]; }
        // a point farther than 0.1 from the box of all of q's vertices is an outlier without any search
        const bool search = on && x >= box[0] && y >= box[1] && z >= box[2] && x <= box[3] && y <= box[4] && z <= box[5];
        float best = -1.0f;
        int bi = INT_MAX;
        if (__any(search)) knn_capped(vs, cb, x, y, z, search ? cap2 : -1.0f, best, bi);      // idle lanes open no cluster
        if (on) {
            // outlier = sqrt(min(d2, 4)) > 0.1 (deformer.py:41-49), the rule of k_warp_inverse
            const bool is_out = bi == INT_MAX || sqrtf(fminf(best, 4.0f)) > 0.1f;
            probed[row0 + i] = is_out ? 0 : 1;
            if (!is_out) {
                const float4 r0 = bt[3 * bi], r1 = bt[3 * bi + 1], r2 = bt[3 * bi + 2];
                const float qx = x - r0.w, qy = y - r1.w, qz = z - r2.w;
                float* o = xc + 3 * (row0 + i);
                o[0] = r0.x * qx + r0.y * qy + r0.z * qz;
                o[1] = r1.x * qx + r1.y * qy + r1.z * qz;
                o[2] = r2.x * qx + r2.y * qy + r2.z * qz;
                nn[row0 + i] = bi;
            }
        }
    }
}

// one block per pair: the probed point ids in ascending order (ballot + prefix over the block's 16 waves, chunk after chunk)
__global__ __launch_bounds__(COMPACT_THREADS) void k_pen_compact(const unsigned char* __restrict__ probed, int P, int n,
                                                                 int* __restrict__ list, int* __restrict__ count) {
    __shared__ int wtot[COMPACT_THREADS / 64];
    const int pair = blockIdx.x, p = pair / P, q = pair - p * P;
    if (p == q) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row0 = (size_t)pair * n;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += COMPACT_THREADS) {
        const int i = c0 + threadIdx.x;
        const bool f = i < n && probed[row0 + i] != 0;
        const unsigned long long m = __ballot(f);
        if (lane == 0) wtot[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
            const int t = wtot[w];
            before += w < wave ? t : 0;
            total += t;
        }
        if (f) list[row0 + base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[pair] = base;
}

// one block per pair; every thread sums a fixed subset of the entries in double, the block adds the 256 partial sums as a tree
__global__ __launch_bounds__(TB) void k_pen_loss(const float* const* __restrict__ sdf_tab, const int* __restrict__ count, int P,
                                                 int n, float* __restrict__ loss, int* __restrict__ active,
                                                 float* const* __restrict__ seed_tab) {
    __shared__ double sacc[TB];
    __shared__ int sact[TB];
    const int pair = blockIdx.x, p = pair / P, q = pair - p * P;
    if (p == q) {
        if (threadIdx.x == 0) { loss[pair] = 0.f; active[pair] = 0; }
        return;
    }
    const float* __restrict__ s = sdf_tab[pair];
    float* __restrict__ seed = seed_tab[pair];
    const int c = (s && seed) ? min(max(count[pair], 0), n) : 0;      // (a pair without entries may carry NULL)
    double acc = 0.0;
    int na = 0;
    for (int e = threadIdx.x; e < c; e += TB) {
        const float v = s[e];
        const bool a = v < 0.f;
        seed[e] = a ? 2.0f * v : 0.f;
        if (a) { acc += (double)v * (double)v; ++na; }
    }
    sacc[threadIdx.x] = acc;
    sact[threadIdx.x] = na;
    __syncthreads();
    for (int o = TB / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) { sacc[threadIdx.x] += sacc[threadIdx.x + o]; sact[threadIdx.x] += sact[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { loss[pair] = (float)sacc[0]; active[pair] = sact[0]; }
}

// grid (vertex blocks, P): one thread per vertex v of the probing person p; partners q ascending, entries ascending.  The block
// stages the vertex ids of 256 entries in LDS and every thread looks for its own.
__global__ __launch_bounds__(TB) void k_pen_scatter_bwd(const int* const* __restrict__ idx_tab, const int* __restrict__ list,
                                                        const int* __restrict__ count, const int* __restrict__ nn,
                                                        const float* const* __restrict__ bt_tab,
                                                        const float* const* __restrict__ dxc_tab, int P, int n, int V,
                                                        float* const* __restrict__ dverts_tab) {
    __shared__ int sv[TB];
    const int p = blockIdx.y, v = blockIdx.x * TB + threadIdx.x;
    const int* __restrict__ idx = idx_tab[p];
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    for (int q = 0; q < P; ++q) {
        if (q == p) continue;
        const int pair = p * P + q;
        const int c = min(max(count[pair], 0), n);
        const size_t row0 = (size_t)pair * n;
        const float* __restrict__ dxc = dxc_tab[pair];
        const float4* __restrict__ bt = (const float4*)bt_tab[q];
        for (int e0 = 0; e0 < c; e0 += TB) {
            __syncthreads();
            const int e = e0 + threadIdx.x;
            int drawn = -1;
            if (e < c) {
                const int i = list[row0 + e];
                if (i >= 0 && i < n) drawn = idx[i];
            }
            sv[threadIdx.x] = drawn;
            __syncthreads();
            const int m = min(TB, c - e0);
            for (int j = 0; j < m; ++j) {
                if (sv[j] != v) continue;
                const int b = nn[row0 + list[row0 + e0 + j]];
                if (b < 0 || b >= V) continue;
                const float4 r0 = bt[3 * b], r1 = bt[3 * b + 1], r2 = bt[3 * b + 2];
                const float* g = dxc + 3 * (size_t)(e0 + j);
                d0 += r0.x * g[0] + r1.x * g[1] + r2.x * g[2];
                d1 += r0.y * g[0] + r1.y * g[1] + r2.y * g[2];
                d2 += r0.z * g[0] + r1.z * g[1] + r2.z * g[2];
            }
        }
    }
    if (v < V) {
        float* o = dverts_tab[p] + 3 * (size_t)v;
        o[0] += d0; o[1] += d1; o[2] += d2;
    }
}

bool persons_ok(int P) { return P >= 2 && P <= mp::MAX_P; }

}  // namespace

extern "C" int mp_pen_probe(const float* const* pts, const float* const* vsorted, const float* const* cbound,
                            const float* const* blend_table, int n_person, int n, unsigned char* probed, int* nn, float* xc,
                            int* list, int* count, void* stream) {
    if (n < 0 || !persons_ok(n_person) || !pts || !vsorted || !cbound || !blend_table || !probed || !nn || !xc || !list || !count)
        return -1;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    MP_LDS_ATTR((k_pen_probe), PROBE_LDS);
    const int n_slab = (n + 63) / 64, nw = PROBE_THREADS / 64;
    hipLaunchKernelGGL(k_pen_probe, dim3((n_slab + nw - 1) / nw, n_person * n_person), dim3(PROBE_THREADS), PROBE_LDS, st, pts,
                       vsorted, cbound, blend_table, n_person, n, probed, nn, xc);
    hipLaunchKernelGGL(k_pen_compact, dim3(n_person * n_person), dim3(COMPACT_THREADS), 0, st, (const unsigned char*)probed,
                       n_person, n, list, count);
    return (int)hipGetLastError();
}

extern "C" int mp_pen_loss(const float* const* sdf, const int* count, int n_person, int n, float* loss, int* active,
                           float* const* seed, void* stream) {
    if (n < 0 || !persons_ok(n_person) || !sdf || !count || !loss || !active || !seed) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_pen_loss, dim3(n_person * n_person), dim3(TB), 0, (hipStream_t)stream, sdf, count, n_person, n, loss,
                       active, seed);
    return (int)hipGetLastError();
}

extern "C" int mp_pen_scatter_bwd(const int* const* pen_idx, const int* list, const int* count, const int* nn,
                                  const float* const* blend_table, const float* const* dxc, int n_person, int n, int n_verts,
                                  float* const* dverts, void* stream) {
    if (n < 0 || n_verts < 0 || !persons_ok(n_person) || !pen_idx || !list || !count || !nn || !blend_table || !dxc || !dverts)
        return -1;
    if (n == 0 || n_verts == 0) return 0;
    hipLaunchKernelGGL(k_pen_scatter_bwd, dim3((n_verts + TB - 1) / TB, n_person), dim3(TB), 0, (hipStream_t)stream, pen_idx,
                       list, count, nn, blend_table, dxc, n_person, n, n_verts, dverts);
    return (int)hipGetLastError();
}
