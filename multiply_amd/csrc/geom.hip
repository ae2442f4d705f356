// Geometry kernels: nearest-vertex structure, blend table and the canonical warp (SMPL posing: smpl.hip; rays and culling:
// rays.hip; oriented boxes and the convex hull: obb.hip).
// Entry points and the reference code they replace: include/multiply_hip.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"

namespace {

constexpr int V = MP_SMPL_V, NJ = MP_SMPL_J, NC = MP_KNN_NC, CL = MP_KNN_CLUSTER;
constexpr int NCC = MP_KNN_NC / 2, CLC = 2 * MP_KNN_CLUSTER;      // the coarse granularity of the training searches: pairs of clusters (k_knn_build)
static_assert(MP_KNN_NC % 2 == 0 && 2 * MP_KNN_CLUSTER <= 64, "coarse clusters = pairs of fine ones, one wave each");
__host__ __device__ constexpr int mp_fine_clusters() { return MP_KNN_NC; }      // (where a local NC shadows the fine count)

// ------------------------------------------------------------------------------------------------ KNN structure
// Blocks NC .. NC + NCC - 1 (round 6): the bounding sphere of the PAIR of clusters (2 cc, 2 cc + 1) -- consecutive kd leaves, siblings --
// as cbound[NC + cc].  The training searches (every sample of a ray needs its exact neighbour however far away it is, so many
// spheres are about equally near) run on these NCC = NC / 2 coarse clusters of 2 CL vertices: with the fine ones the training
// warp cost +30 % (twice the sphere tests and per-cluster steps), the eval searches -19 % (profiles/r06_cluster_ab.txt).
__global__ __launch_bounds__(64) void k_knn_build(const float* __restrict__ verts, const int* __restrict__ perm,
                                                  float4* __restrict__ vsorted, float4* __restrict__ cbound) {
    const int l = threadIdx.x;
    if (blockIdx.x >= NC) {
        const int cc = blockIdx.x - NC;
        const int id = l < 2 * CL ? perm[cc * 2 * CL + l] : -1;
        float x = 0.f, y = 0.f, z = 0.f;
        if (id >= 0) { x = verts[3 * id]; y = verts[3 * id + 1]; z = verts[3 * id + 2]; }
        const float n = fmaxf(mp::wsum(id >= 0 ? 1.f : 0.f), 1.f);      // (an all-padding cluster: a zero sphere at the origin)
        const float cx = mp::wsum(x) / n, cy = mp::wsum(y) / n, cz = mp::wsum(z) / n;
        const float dx = x - cx, dy = y - cy, dz = z - cz;
        const float r = mp::wmax(id >= 0 ? sqrtf(dx * dx + dy * dy + dz * dz) : 0.f);
        if (l == 0) cbound[NC + cc] = make_float4(cx, cy, cz, r * 1.00001f + 1e-7f);
        return;
    }
    const int c = blockIdx.x;                           // one full wave per cluster; lanes >= CL (CL < 64) hold padding
    const int id = l < CL ? perm[c * CL + l] : -1;
    float x = 0.f, y = 0.f, z = 0.f;
    if (id >= 0) { x = verts[3 * id]; y = verts[3 * id + 1]; z = verts[3 * id + 2]; }
    const float n = fmaxf(mp::wsum(id >= 0 ? 1.f : 0.f), 1.f);      // (an all-padding cluster: a zero sphere at the origin)
    const float cx = mp::wsum(x) / n, cy = mp::wsum(y) / n, cz = mp::wsum(z) / n;
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float r = mp::wmax(id >= 0 ? sqrtf(dx * dx + dy * dy + dz * dz) : 0.f);
    float4 o;
    if (id >= 0) { o.x = x; o.y = y; o.z = z; o.w = __int_as_float(id); }
    else { o.x = 1e18f; o.y = 1e18f; o.z = 1e18f; o.w = __int_as_float(INT_MAX - 1); }
    if (l < CL) vsorted[c * CL + l] = o;
    if (l == 0) cbound[c] = make_float4(cx, cy, cz, r * 1.00001f + 1e-7f);
}
}  // namespace

extern "C" int mp_knn_build(const float* verts, const int* perm, float* vsorted, float* cbound, void* stream) {
    hipLaunchKernelGGL(k_knn_build, dim3(NC + NCC), dim3(64), 0, (hipStream_t)stream, verts, perm, (float4*)vsorted,
                       (float4*)cbound);
    return (int)hipGetLastError();
}

namespace {
// -DMP_GEOM_PROF: cycle / event counters of the warp kernels, summed over waves (tools/geom_prof.py reads them):
//  [0] slabs  [1] cycles total  [2] cycles in knn cull (reductions + sphere tests)  [3] cycles in cluster scans
//  [4] clusters that passed the box cull  [5] clusters scanned  [6] cycles in loads  [7] cycles in the epilogue
#ifdef MP_GEOM_PROF
__device__ unsigned long long g_geom_prof[16];
#define GP_T() __builtin_readcyclecounter()
__shared__ unsigned long long gp_lds[16][16];   // per-wave accumulators: one global atomic per wave and counter at exit
#define GP_ADD(i, v) do { if ((threadIdx.x & 63) == 0) gp_lds[threadIdx.x >> 6][i] += (unsigned long long)(v); } while (0)
#define GP_BEGIN() do { if ((threadIdx.x & 63) < 16) gp_lds[threadIdx.x >> 6][threadIdx.x & 63] = 0; } while (0)
#define GP_END() do { if ((threadIdx.x & 63) < 16) atomicAdd(&g_geom_prof[threadIdx.x & 63], gp_lds[threadIdx.x >> 6][threadIdx.x & 63]); } while (0)
extern "C" int mp_geom_prof_read(unsigned long long* host16, int reset) {
    hipError_t e = hipMemcpyFromSymbol(host16, HIP_SYMBOL(g_geom_prof), sizeof(unsigned long long) * 16);
    if (reset) { unsigned long long z[16] = {0}; hipMemcpyToSymbol(HIP_SYMBOL(g_geom_prof), z, sizeof(z)); }
    return (int)e;
}
#else
#define GP_T() 0ull
#define GP_ADD(i, v) do { } while (0)
#define GP_BEGIN() do { } while (0)
#define GP_END() do { } while (0)
#endif
}  // namespace

#include "knn_search.hpp"      // knn_capped, load_knn_lds (with the counters above under -DMP_GEOM_PROF)

namespace {
// Unbounded exact search.  An upper bound of the nearest-vertex distance is cheap: every cluster's bounding sphere
// contains at least one vertex, so d_nn <= min_c (|p - centre_c| + radius_c)  (NC broadcast LDS reads per lane).  With
// that per-lane cap a single culled pass finds the exact neighbour of near and far points alike (the previous scheme,
// growing a fixed cap geometrically, re-culled the clusters up to 7 times for the far samples of a training ray).
// want: lane participates.
template <bool NEAR_FIRST, int NCX = NC, int CLX = CL>
__device__ __forceinline__ void knn_unbounded(const float4* vs, const float4* cb, float px, float py, float pz, bool want,
                                              float& best, int& bi) {
    constexpr int NC = NCX, CL = CLX;
    best = -1.0f;
    bi = INT_MAX;
    bool todo = want;
    if constexpr (NEAR_FIRST) {   // canonical shading points sit near the surface: growing fixed radii resolve them fastest
        float cap = 0.0064f;      // (0.08)^2, then (0.16)^2, (0.32)^2
        for (int round = 0; round < 3 && __any(todo); ++round) {
            float b2; int i2;
            knn_capped<NC, CL>(vs, cb, px, py, pz, todo ? cap : -1.0f, b2, i2);
            if (todo && i2 != INT_MAX) { best = b2; bi = i2; todo = false; }
            cap *= 4.0f;
        }
    }
    if (__any(todo)) {
        float ub = FLT_MAX;
        for (int c = 0; c < NC; ++c) {
            const float4 b = cb[c];
            const float ex = px - b.x, ey = py - b.y, ez = pz - b.z;
            ub = fminf(ub, sqrtf(ex * ex + ey * ey + ez * ez) + b.w);
        }
        float b2; int i2;
        knn_capped<NC, CL>(vs, cb, px, py, pz, todo ? ub * ub * 1.0005f + 1e-12f : -1.0f, b2, i2);
        if (todo) { best = b2; bi = i2; }
    }
}

// blended bone transform rows 0..2 (T[12]) and T[3][3] (s) of vertex `vid`
__device__ __forceinline__ void blend_tf(const float* __restrict__ skin_w, const float* tfs_lds, int vid, float (&T)[12],
                                         float& s33) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
    s33 = 0.f;
    const float* w = skin_w + (size_t)vid * NJ;
    for (int j = 0; j < NJ; ++j) {
        const float wj = w[j];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] += wj * tfs_lds[16 * j + i];
        s33 += wj * tfs_lds[16 * j + 15];
    }
}

__device__ __forceinline__ void inv3(const float (&T)[12], float (&I)[9]) {
    const float a = T[0], b = T[1], c = T[2], d = T[4], e = T[5], f = T[6], g = T[8], h = T[9], i = T[10];
    const float c0 = e * i - f * h, c1 = f * g - d * i, c2 = d * h - e * g;
    const float det = a * c0 + b * c1 + c * c2;
    const float r = 1.0f / det;
    I[0] = c0 * r; I[1] = (c * h - b * i) * r; I[2] = (b * f - c * e) * r;
    I[3] = c1 * r; I[4] = (a * i - c * g) * r; I[5] = (c * d - a * f) * r;
    I[6] = c2 * r; I[7] = (b * g - a * h) * r; I[8] = (a * e - b * d) * r;
}

// Per-vertex inverse blended transform of one pose: row r of vertex v = (I[3r], I[3r+1], I[3r+2], T[r][3] / T[3][3]) with
// T = sum_j w[v][j] tfs[j] and I = inverse of its 3x3 block.  The warp kernels map a point whose nearest vertex is v with
// x_c = I (x - c): one 48-byte gather per point instead of 24 scattered weight loads, 312 FMAs and a 3x3 inversion, with
// the same operations in the same order (the table is what every point with that neighbour computed for itself before).
__global__ void k_blend_table(const float* __restrict__ skin_w, const float* __restrict__ tfs, int n_verts,
                              float4* __restrict__ table) {
    __shared__ float tl[NJ * 16];
    for (int i = threadIdx.x; i < NJ * 16; i += blockDim.x) tl[i] = tfs[i];
    __syncthreads();
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_verts) return;
    float T[12], s33, I[9];
    blend_tf(skin_w, tl, v, T, s33);
    inv3(T, I);
    table[3 * v] = make_float4(I[0], I[1], I[2], T[3] / s33);
    table[3 * v + 1] = make_float4(I[3], I[4], I[5], T[7] / s33);
    table[3 * v + 2] = make_float4(I[6], I[7], I[8], T[11] / s33);
}
}  // namespace

extern "C" int mp_blend_table(const float* skin_w, const float* tfs, int n_verts, float* table, void* stream) {
    if (n_verts <= 0) return 0;
    hipLaunchKernelGGL(k_blend_table, dim3((n_verts + 255) / 256), dim3(256), 0, (hipStream_t)stream, skin_w, tfs, n_verts,
                       (float4*)table);
    return (int)hipGetLastError();
}

namespace {
constexpr int WARP_THREADS = 1024;
constexpr int WARP_LDS = NC * CL * 16 + (NC + NCC) * 16 + 32;      // vertices, fine + coarse spheres, box
// k_warp_inverse appends the ids of the points that need a network query to ONE list.  One returning atomicAdd per slab on that list's
// counter was the kernel: 624 k same-address atomics per frame serialise in one L2 channel (shading launches 4.75 ms, 2.30 ms with the
// atomic removed; profiles/r06_worklist_atomic.txt).  Every wave therefore stages ids in its own strip of LDS and reserves list space
// once per WL_STAGE - 64 ids or more (~8 slabs).
constexpr int WL_STAGE = 512;
constexpr int WARP_INV_LDS = WARP_LDS + (WARP_THREADS / 64) * WL_STAGE * 4;

// Which 64 (ray, sample) pairs share a wave of a rays-mode launch.  Rounds 1-5: 64 neighbouring rays x one sample index.  The per-point
// outputs are addressed [ray][sample], so every store instruction of such a wave touches 64 cache lines; the shading launch (mode 2: xc,
// flags, nearest-vertex index, and after it the Jacobian's 36 bytes per point) therefore takes MP_SLAB_RUN consecutive samples of 64 /
// MP_SLAB_RUN neighbouring rays (round 6) -- runs share their lines, the points stay as compact in space (pixels of a tile row x a short
// stretch of depth).  The sampler's launches (modes 0 / 1) write one value per point and measured slower that way: they keep 64 x 1.
#ifndef MP_SLAB_RUN
#define MP_SLAB_RUN 8
#endif
#ifndef MP_SLAB_RUN_SAMPLER
#define MP_SLAB_RUN_SAMPLER 1
#endif
__host__ __device__ constexpr int slab_run(int mode) { return mode == 2 ? MP_SLAB_RUN : MP_SLAB_RUN_SAMPLER; }

// one wave: reserve `staged` entries of the list and copy the wave's strip there (wave-private LDS: in order, no barrier)
__device__ __forceinline__ void worklist_flush(const int* stage, int staged, int* __restrict__ worklist, int* __restrict__ work_count, int lane) {
    int base = 0;
    if (lane == 0) base = atomicAdd(work_count, staged);
    base = __shfl(base, 0);
    for (int i = lane; i < staged; i += 64) worklist[base + i] = stage[i];
}

// mode 0: all points -> xc + worklist; mode 1: eval, outliers get sdf 4 and are skipped;
// mode 2: eval shading, outliers get sdf 4 and are skipped only when their alpha is exactly 0 in fp32
__global__ __launch_bounds__(WARP_THREADS) void k_warp_inverse(
    const float* __restrict__ pts, const float* __restrict__ dirs, const float* __restrict__ pose,
    const int* __restrict__ hit_index, const int* __restrict__ hit_count, const float* __restrict__ z, int z_stride,
    int n_s, int max_rays, int n_pts, const float* __restrict__ vsorted, const float* __restrict__ cbound,
    const float4* __restrict__ btab, int mode, const int* __restrict__ ray_active,
    const float* __restrict__ beta_p, const int* __restrict__ launch_active, float* __restrict__ xc,
    unsigned char* __restrict__ outlier, unsigned char* __restrict__ need_flag, float* __restrict__ sdf_out,
    int* __restrict__ worklist, int* __restrict__ work_count, int* __restrict__ nn_index,
    const float4* __restrict__ binned, const int* __restrict__ bincount) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (launch_active && *launch_active == 0) return;  // no ray of this launch is still being sampled
    float4* vs = (float4*)smem;
    float4* cb = vs + NC * CL;
    float4* cbc = cb + NC;           // the coarse spheres (training searches)
    float* box = (float*)(cbc + NCC);  // [6] conservative bounds of the vertex set (from the cluster spheres)
    int* stage = (int*)(smem + WARP_LDS) + (threadIdx.x >> 6) * WL_STAGE;   // this wave's strip of list entries not yet written out
    int staged = 0;
    load_knn_lds(vs, cb, vsorted, cbound);
    if (mode == 0) for (int i = threadIdx.x; i < NCC; i += blockDim.x) cbc[i] = ((const float4*)cbound)[NC + i];
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
    GP_BEGIN();
    const bool rays = pts == nullptr && binned == nullptr;
    const int n_rays = rays ? min(*hit_count, max_rays) : 0;
    if (binned) {          // the points in the order of k_warp_bin / k_warp_binned: n_pts = how many there are
        n_pts = 0;
        for (int c = 0; c < NCC; ++c) n_pts += bincount[c];
    }
    const int run = slab_run(mode), n_sr = (n_s + run - 1) / run, rpw = 64 / run;       // samples per run, runs per ray, rays per wave
    const int n_slab = rays ? ((n_rays + rpw - 1) / rpw) * n_sr : (n_pts + 63) / 64;
    float cam[3] = {0.f, 0.f, 0.f};
    if (rays) { cam[0] = pose[3]; cam[1] = pose[7]; cam[2] = pose[11]; }
    const float cap2 = 0.0101f;  // eval only needs neighbours within the 0.1 outlier radius
    for (int slab = blockIdx.x * nw + wave; slab < n_slab; slab += gridDim.x * nw) {
        int pid = -1;
        float x = 0.f, y = 0.f, zz = 0.f, dt = 0.f;
        const unsigned long long gs0 = GP_T();
        GP_ADD(0, 1);
        if (rays) {
            const int rb = slab / n_sr, k = rb * rpw + lane / run, s = (slab - rb * n_sr) * run + lane % run;
            if (k < n_rays && s < n_s && (!ray_active || ray_active[k])) {
                const int r = hit_index[k];
                const float t = z[(size_t)k * z_stride + s];
                x = cam[0] + t * dirs[3 * r]; y = cam[1] + t * dirs[3 * r + 1]; zz = cam[2] + t * dirs[3 * r + 2];
                pid = k * n_s + s;
                if (mode == 2) dt = z[(size_t)k * z_stride + s + 1] - t;
            }
        } else if (binned) {
            const int i = slab * 64 + lane;
            if (i < n_pts) { const float4 q = binned[i]; x = q.x; y = q.y; zz = q.z; pid = __float_as_int(q.w); }
        } else {
            const int i = slab * 64 + lane;
            if (i < n_pts) { x = pts[3 * i]; y = pts[3 * i + 1]; zz = pts[3 * i + 2]; pid = i; }
        }
        // eval: a point farther than 0.1 from the box of all vertices is an outlier without any search
        const bool near_box = mode == 0 || (x >= box[0] && y >= box[1] && zz >= box[2] && x <= box[3] && y <= box[4] &&
                                            zz <= box[5]);
        float best = -1.0f;
        int bi = INT_MAX;
#ifdef MP_GEOM_PROF
        x += __int_as_float(__float_as_int(x) & 0);   // keep the loads ahead of the stamp
        const unsigned long long gs1 = GP_T();
        GP_ADD(6, gs1 - gs0);
#endif
        if (mode == 0) knn_unbounded<false, NCC, CLC>(vs, cbc, x, y, zz, pid >= 0, best, bi);
        else if (__any(pid >= 0 && near_box))
            knn_capped(vs, cb, x, y, zz, (pid >= 0 && near_box) ? cap2 : -1.0f, best, bi);  // idle lanes open no cluster
        bool append = false, need_far = false, need = false, is_out = false;
        if (pid >= 0) {
            // outlier = sqrt(min(d2, 4)) > 0.1 (deformer.py:41-49)
            is_out = bi == INT_MAX || sqrtf(fminf(best, 4.0f)) > 0.1f;
            if (outlier) outlier[pid] = is_out ? 1 : 0;
            need = true;
            if (mode != 0 && is_out) {
                sdf_out[pid] = 4.0f;  // multiply.py:142-143
                need = false;
                if (mode == 2) {  // keep it only if its compositing weight can be non-zero
                    need = mp::alpha_of(4.0f, *beta_p, dt) != 0.0f;
                }
            }
            need_far = need && bi == INT_MAX;   // rare: outlier that still has weight -> exact unbounded search below
        }
        if (__any(need_far)) {
            float b2; int i2;
            knn_unbounded<false>(vs, cb, x, y, zz, need_far, b2, i2);
            if (need_far) { best = b2; bi = i2; }
        }
        const unsigned long long gs2 = GP_T();
        if (pid >= 0) {
            if (need_flag) need_flag[pid] = need ? 1 : 0;
            if (need) {
                const float4 r0 = btab[3 * bi], r1 = btab[3 * bi + 1], r2 = btab[3 * bi + 2];
                const float qx = x - r0.w, qy = y - r1.w, qz = zz - r2.w;
                xc[3 * (size_t)pid] = r0.x * qx + r0.y * qy + r0.z * qz;
                xc[3 * (size_t)pid + 1] = r1.x * qx + r1.y * qy + r1.z * qz;
                xc[3 * (size_t)pid + 2] = r2.x * qx + r2.y * qy + r2.z * qz;
                if (nn_index) nn_index[pid] = bi;
                append = worklist != nullptr;
            }
        }
        if (worklist) {
            const unsigned long long m = __ballot(append);
            if (m) {
                if (append) stage[staged + __popcll(m & ((1ull << lane) - 1ull))] = pid;
                staged += __popcll(m);
                if (staged > WL_STAGE - 64) { worklist_flush(stage, staged, worklist, work_count, lane); staged = 0; }
            }
        }
#ifdef MP_GEOM_PROF
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long gs3 = GP_T();
        GP_ADD(7, gs3 - gs2);
        GP_ADD(1, gs3 - gs0);
#endif
    }
    if (staged) worklist_flush(stage, staged, worklist, work_count, lane);
    GP_END();
}

// ---- TRAINING: the points of a wave grouped by their nearest vertex cluster -----------------------------------------------------
// A training batch is 512 RANDOM pixels: the 64 hit rays of a slab are scattered over the body's box, and most samples of a ray
// lie in free space far from the surface, where many clusters are about equally far.  The cluster scan is wave-uniform (a
// cluster is scanned when ANY lane may improve in it), so such a slab opened 50 of the (then 108) clusters (measured: 226 k cycles per
// slab, 1.15 ms per iteration).  Which 64 points share a wave is the kernel's own business -- results go out by point id -- so
// the points are first binned by the cluster whose bounding sphere is nearest (k_warp_bin: one atomic per point gives bin and
// rank), laid out bin after bin (k_warp_binned: position, point id), and k_warp_inverse walks that array.
__device__ __forceinline__ bool warp_sample_point(const float* dirs, const float* pose, const int* hit_index, const float* z,
                                                  int z_stride, int n_s, int n_rays, const int* ray_active, int i, float& x, float& y,
                                                  float& zz) {
    if (i >= n_rays * n_s) return false;
    const int k = i / n_s, s = i - k * n_s;
    if (ray_active && !ray_active[k]) return false;
    const int r = hit_index[k];
    const float t = z[(size_t)k * z_stride + s];
    x = pose[3] + t * dirs[3 * r]; y = pose[7] + t * dirs[3 * r + 1]; zz = pose[11] + t * dirs[3 * r + 2];
    return true;
}
__global__ __launch_bounds__(1024) void k_warp_bin(const float* __restrict__ dirs, const float* __restrict__ pose,
                                                   const int* __restrict__ hit_index, const int* __restrict__ hit_count,
                                                   const float* __restrict__ z, int z_stride, int n_s, int max_rays,
                                                   const float* __restrict__ cbound, const int* __restrict__ ray_active,
                                                   const int* __restrict__ launch_active, int* __restrict__ binrank,
                                                   int* __restrict__ bincount) {
    if (launch_active && *launch_active == 0) return;
    constexpr int NC = NCC;                    // bins = the coarse clusters the binned walk searches
    __shared__ float4 cb[NC];
    __shared__ int lcount[NC], lbase[NC];      // this workgroup's histogram, then its base rank in every bin
    for (int i = threadIdx.x; i < NC; i += blockDim.x) { cb[i] = ((const float4*)cbound)[mp_fine_clusters() + i]; lcount[i] = 0; }
    __syncthreads();
    const int n_rays = min(*hit_count, max_rays);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    float x, y, zz;
    const bool on = warp_sample_point(dirs, pose, hit_index, z, z_stride, n_s, n_rays, ray_active, i, x, y, zz);
    int bc = 0, lrank = 0;
    if (on) {
        float best = FLT_MAX;
        for (int c = 0; c < NC; ++c) {
            const float4 b = cb[c];
            const float ex = x - b.x, ey = y - b.y, ez = zz - b.z;
            const float gap = sqrtf(ex * ex + ey * ey + ez * ez) - b.w;
            if (gap < best) { best = gap; bc = c; }
        }
        lrank = atomicAdd(&lcount[bc], 1);     // (LDS: the global counters see one add per workgroup and bin, not one per point --
    }                                          //  60 k same-address atomics on ~100 words took 110 us)
    __syncthreads();
    for (int c = threadIdx.x; c < NC; c += blockDim.x) lbase[c] = lcount[c] ? atomicAdd(&bincount[c], lcount[c]) : 0;
    __syncthreads();
    if (on) binrank[i] = (bc << 22) | (lbase[bc] + lrank);      // bin (< 512) | rank inside the bin (< 4 M points per launch); -1 = none
    else if (i < max_rays * n_s) binrank[i] = -1;
}
__global__ __launch_bounds__(256) void k_warp_binned(const float* __restrict__ dirs, const float* __restrict__ pose,
                                                     const int* __restrict__ hit_index, const int* __restrict__ hit_count,
                                                     const float* __restrict__ z, int z_stride, int n_s, int max_rays,
                                                     const int* __restrict__ launch_active, const int* __restrict__ binrank,
                                                     const int* __restrict__ bincount, float4* __restrict__ binned) {
    if (launch_active && *launch_active == 0) return;
    constexpr int NC = NCC;
    __shared__ int start[NC];
    if (threadIdx.x == 0) {
        int a = 0;
        for (int c = 0; c < NC; ++c) { start[c] = a; a += bincount[c]; }
    }
    __syncthreads();
    const int n_rays = min(*hit_count, max_rays);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rays * n_s) return;
    const int br = binrank[i];
    if (br < 0) return;
    float x, y, zz;
    warp_sample_point(dirs, pose, hit_index, z, z_stride, n_s, n_rays, nullptr, i, x, y, zz);
    binned[start[br >> 22] + (br & 0x3fffff)] = make_float4(x, y, zz, __int_as_float(i));
}

// Points are addressed like in k_warp_inverse (slab = 64 neighbouring hit rays x one sample index, so the 64 canonical
// points of a wave are spatially coherent); only points whose `need` flag is set are processed.
// Explicit-list variant (n_s == 0): point id = index, all `count` points processed.
__global__ __launch_bounds__(WARP_THREADS) void k_warp_jacobian(const float* __restrict__ xc,
                                                                const unsigned char* __restrict__ need,
                                                                const int* __restrict__ hit_count, int max_rays, int n_s,
                                                                int n_pts, const float* __restrict__ vsorted_c,
                                                                const float* __restrict__ cbound_c,
                                                                const float4* __restrict__ btab,
                                                                float* __restrict__ jinv,
                                                                int* __restrict__ nn_index,
                                                                const int* __restrict__ seed,
                                                                const float* __restrict__ verts_c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* vs = (float4*)smem;
    float4* cb = vs + NC * CL;
    load_knn_lds(vs, cb, vsorted_c, cbound_c);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    GP_BEGIN();
    const bool rays = n_s > 0;
    const int n_rays = rays ? min(*hit_count, max_rays) : 0;
    const int run = slab_run(2), n_sr = (n_s + run - 1) / run, rpw = 64 / run;          // (the shading launch's mapping, see k_warp_inverse)
    const int n_slab = rays ? ((n_rays + rpw - 1) / rpw) * n_sr : (n_pts + 63) / 64;
    for (int slab = blockIdx.x * nw + wave; slab < n_slab; slab += gridDim.x * nw) {
        int id = -1;
        if (rays) {
            const int rb = slab / n_sr, k = rb * rpw + lane / run, s = (slab - rb * n_sr) * run + lane % run;
            if (k < n_rays && s < n_s && need[(size_t)k * n_s + s]) id = k * n_s + s;
        } else {
            const int i = slab * 64 + lane;
            if (i < n_pts) id = i;
        }
        if (!__any(id >= 0)) continue;
        const unsigned long long gs0 = GP_T();
        GP_ADD(0, 1);
        float x = 0.f, y = 0.f, z = 0.f;
        if (id >= 0) { x = xc[3 * (size_t)id]; y = xc[3 * (size_t)id + 1]; z = xc[3 * (size_t)id + 2]; }
        float best; int bi;
        if (seed) {
            // the nearest POSED vertex of the deformed point is (almost always) also the nearest canonical vertex of x_c:
            // its canonical distance is a tight search radius, so one culled pass over very few clusters is exact
            float cap2 = -1.0f;
            if (id >= 0) {
                const int sv = seed[id];
                const float ex = x - verts_c[3 * sv], ey = y - verts_c[3 * sv + 1], ez = z - verts_c[3 * sv + 2];
                cap2 = (ex * ex + ey * ey + ez * ez) * 1.0005f + 1e-12f;
            }
            knn_capped(vs, cb, x, y, z, cap2, best, bi);
        } else {
            knn_unbounded<true>(vs, cb, x, y, z, id >= 0, best, bi);
        }
        if (id >= 0) {
            const float4 r0 = btab[3 * bi], r1 = btab[3 * bi + 1], r2 = btab[3 * bi + 2];
            float* o = jinv + 9 * (size_t)id;
            o[0] = r0.x; o[1] = r0.y; o[2] = r0.z; o[3] = r1.x; o[4] = r1.y; o[5] = r1.z; o[6] = r2.x; o[7] = r2.y; o[8] = r2.z;
            if (nn_index) nn_index[id] = bi;
        }
#ifdef MP_GEOM_PROF
        __builtin_amdgcn_s_waitcnt(0);
        GP_ADD(1, GP_T() - gs0);
#endif
    }
    GP_END();
}

// waves of work in a rays-mode launch (the kernels' own (ray, sample) -> wave mapping)
int ray_slabs(int max_rays, int n_s, int mode) {
    const int run = slab_run(mode), rpw = 64 / run;
    return ((max_rays + rpw - 1) / rpw) * ((n_s + run - 1) / run);
}

int warp_grid(int n_slab, int nw) {
    int g = (n_slab + nw - 1) / nw;
    return g < 1 ? 1 : (g > 256 ? 256 : g);
}

// Waves per workgroup of the warp kernels.  One workgroup per CU either way (its vertex structure fills 110 KB of LDS);
// 16 waves amortise that fill over a whole frame's slabs, but a training call has only ~900 slabs (512 rays x 128
// samples / 64) and would occupy 57 of the 256 CUs -- there, fewer waves per workgroup spread the slabs over the chip.
int warp_threads(int n_slab) {
    int nw = (n_slab + 255) / 256;          // waves per workgroup that give every CU a workgroup
    nw = nw < 1 ? 1 : (nw > WARP_THREADS / 64 ? WARP_THREADS / 64 : nw);
    return nw * 64;
}

}  // namespace

// bin_work (mp_warp_bin_work_bytes(max_rays * n_s) bytes, 16-byte aligned): [BIN_CNT] bin counts, [n] bin << 22 | rank, [n] float4
constexpr int BIN_CNT = (NCC + 127) / 128 * 128;      // bin counters at the head of the work buffer (a multiple of 512 bytes)
static_assert(NC <= 511 && (CL & (CL - 1)) == 0 && CL <= 64 && NC * CL >= V, "cluster layout (include/multiply_hip.h)");
extern "C" int mp_warp_bin_work_bytes(int n_points) { return 4 * BIN_CNT + 4 * ((n_points + 3) / 4 * 4) + 16 * n_points; }
static void warp_bin(const float* dirs, const float* pose, const int* hit_index, const int* hit_count, const float* z, int z_stride,
                     int n_s, int max_rays, const float* cbound, const int* ray_active, const int* launch_active, void* bin_work,
                     hipStream_t st, const float4*& binned, const int*& bincount) {
    const int n = max_rays * n_s;
    int* cnt = (int*)bin_work;
    int* binrank = cnt + BIN_CNT;
    float4* out = (float4*)((char*)bin_work + 4 * BIN_CNT + 4 * ((n + 3) / 4 * 4));
    hipMemsetAsync(cnt, 0, 4 * BIN_CNT, st);
    hipLaunchKernelGGL(k_warp_bin, dim3((n + 1023) / 1024), dim3(1024), 0, st, dirs, pose, hit_index, hit_count, z, z_stride, n_s, max_rays,
                       cbound, ray_active, launch_active, binrank, cnt);
    hipLaunchKernelGGL(k_warp_binned, dim3((n + 255) / 256), dim3(256), 0, st, dirs, pose, hit_index, hit_count, z, z_stride, n_s,
                       max_rays, launch_active, (const int*)binrank, (const int*)cnt, out);
    binned = out;
    bincount = cnt;
}

extern "C" int mp_warp_inverse(const float* pts, const float* dirs, const float* pose, const int* hit_index,
                               const int* hit_count, const float* z, int z_stride, int n_s, int max_rays,
                               const float* vsorted, const float* cbound, const float* blend_table,
                               int mode, const int* ray_active, const int* launch_active, float* xc,
                               unsigned char* outlier, float* sdf_out, int* worklist, int* work_count, void* bin_work,
                               void* stream) {
    // when pts != NULL, max_rays carries the number of explicit points and sdf_out may carry beta for mode 2 (unused)
    if (max_rays <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    MP_LDS_ATTR((k_warp_inverse), WARP_INV_LDS);
    const int n_slab = pts ? (max_rays + 63) / 64 : ray_slabs(max_rays, n_s, mode & 3);
    const int threads = warp_threads(n_slab), nw = threads / 64;
    const float4* binned = nullptr;
    const int* bincount = nullptr;
    if (bin_work && !pts && (mode & 3) == 0) warp_bin(dirs, pose, hit_index, hit_count, z, z_stride, n_s, max_rays, cbound, ray_active,
                                                      launch_active, bin_work, st, binned, bincount);
    hipLaunchKernelGGL(k_warp_inverse, dim3(warp_grid(n_slab, nw)), dim3(threads), WARP_INV_LDS, st, pts, dirs, pose,
                       hit_index, hit_count, z, z_stride, n_s, max_rays, pts ? max_rays : 0, vsorted, cbound,
                       (const float4*)blend_table, mode & 3, ray_active, (const float*)nullptr, launch_active, xc, outlier, (unsigned char*)nullptr, sdf_out,
                       worklist, work_count, (int*)nullptr, binned, bincount);
    return (int)hipGetLastError();
}

// eval-shading variant (mode 2) needs beta; exported separately to keep mp_warp_inverse's signature small
extern "C" int mp_warp_inverse_shade(const float* dirs, const float* pose, const int* hit_index, const int* hit_count,
                                     const float* z, int z_stride, int n_s, int max_rays, const float* vsorted,
                                     const float* cbound, const float* blend_table, int eval_mode,
                                     const float* beta, float* xc, unsigned char* outlier, unsigned char* need_flag,
                                     float* sdf_out, int* worklist, int* work_count, int* nn_index, void* bin_work,
                                     void* stream) {
    if (max_rays <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    MP_LDS_ATTR((k_warp_inverse), WARP_INV_LDS);
    const int n_slab = ray_slabs(max_rays, n_s, eval_mode ? 2 : 0);
    const int threads = warp_threads(n_slab), nw = threads / 64;
    const float4* binned = nullptr;
    const int* bincount = nullptr;
    if (bin_work && !eval_mode) warp_bin(dirs, pose, hit_index, hit_count, z, z_stride, n_s, max_rays, cbound, nullptr, nullptr, bin_work,
                                         st, binned, bincount);
    hipLaunchKernelGGL(k_warp_inverse, dim3(warp_grid(n_slab, nw)), dim3(threads), WARP_INV_LDS, st,
                       (const float*)nullptr, dirs, pose, hit_index, hit_count, z, z_stride, n_s, max_rays, 0, vsorted,
                       cbound, (const float4*)blend_table, eval_mode ? 2 : 0, (const int*)nullptr, beta, (const int*)nullptr, xc, outlier,
                       need_flag, sdf_out, worklist, work_count, nn_index, binned, bincount);
    return (int)hipGetLastError();
}

extern "C" int mp_warp_jacobian(const float* xc, const unsigned char* need, const int* hit_count, int max_rays, int n_s,
                                int n_pts, const float* vsorted_c, const float* cbound_c, const float* blend_table,
                                float* jinv, int* nn_index, const int* seed, const float* verts_c,
                                void* stream) {
    if ((n_s > 0 ? max_rays : n_pts) <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    MP_LDS_ATTR((k_warp_jacobian), WARP_LDS);
    const int n_slab = n_s > 0 ? ray_slabs(max_rays, n_s, 2) : (n_pts + 63) / 64;
    const int threads = warp_threads(n_slab), nw = threads / 64;
    hipLaunchKernelGGL(k_warp_jacobian, dim3(warp_grid(n_slab, nw)), dim3(threads), WARP_LDS, st, xc, need, hit_count,
                       max_rays, n_s, n_pts, vsorted_c, cbound_c, (const float4*)blend_table, jinv, nn_index, seed, verts_c);
    return (int)hipGetLastError();
}
