// Rays: camera rays and their far bound, the box / near-body cull, the flag scan and the ordered compaction of the hit rays.
// Entry points and the reference code they replace: include/multiply_hip.h.
#include <hip/hip_runtime.h>
#include <float.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"

namespace {
constexpr int NC = MP_KNN_NC;
static_assert(MP_KNN_NC <= 511, "cluster layout (include/multiply_hip.h): k_ray_near_body holds the NC fine spheres of cbound in LDS");

// ------------------------------------------------------------------------------------------------ rays
__global__ void k_ray_setup(const float* __restrict__ uv, const float* __restrict__ K, const float* __restrict__ P,
                            int n, float radius, float* __restrict__ dirs, float* __restrict__ far) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float fx = K[0], fy = K[5], cx = K[2], cy = K[6], sk = K[1];
    const float x = uv[2 * i], y = uv[2 * i + 1];
    // lift (rend_util.py:73-87) with z = 1
    const float xl = (x - cx + cy * sk / fy - sk * y / fy) / fx;
    const float yl = (y - cy) / fy;
    float w[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w[a] = P[4 * a] * xl + P[4 * a + 1] * yl + P[4 * a + 2] + P[4 * a + 3];
        d[a] = w[a] - P[4 * a + 3];
    }
    const float nrm = fmaxf(sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), 1e-12f);  // F.normalize
#pragma unroll
    for (int a = 0; a < 3; ++a) { d[a] /= nrm; dirs[3 * i + a] = d[a]; }
    // far root of the bounding sphere (rend_util.py:131-147)
    const float ox = P[3], oy = P[7], oz = P[11];
    const float b = d[0] * ox + d[1] * oy + d[2] * oz;
    const float under = b * b - ((ox * ox + oy * oy + oz * oz) - radius * radius);
    far[i] = fmaxf(sqrtf(under) - b, 0.0f);
}
}  // namespace

extern "C" int mp_ray_setup(const float* uv, const float* intrinsics, const float* pose, int n_rays, float radius,
                            float* dirs, float* far, void* stream) {
    if (n_rays <= 0) return 0;
    hipLaunchKernelGGL(k_ray_setup, dim3((n_rays + 255) / 256), dim3(256), 0, (hipStream_t)stream, uv, intrinsics, pose,
                       n_rays, radius, dirs, far);
    return (int)hipGetLastError();
}

namespace {
__global__ void k_ray_box(const float* __restrict__ dirs, const float* __restrict__ P, const float* __restrict__ obb,
                          int n, int* __restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float o[3] = {P[3] - obb[0], P[7] - obb[1], P[11] - obb[2]};
    const float d[3] = {dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    float tmin = -FLT_MAX, tmax = FLT_MAX;
    bool hit = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float* ax = obb + 3 + 3 * a;
        const float oo = ax[0] * o[0] + ax[1] * o[1] + ax[2] * o[2];
        const float dd = ax[0] * d[0] + ax[1] * d[1] + ax[2] * d[2];
        const float h = obb[12 + a];
        if (fabsf(dd) < 1e-12f) {
            hit = hit && fabsf(oo) <= h;
        } else {
            const float t0 = (-h - oo) / dd, t1 = (h - oo) / dd;
            tmin = fmaxf(tmin, fminf(t0, t1));
            tmax = fminf(tmax, fmaxf(t0, t1));
        }
    }
    flag[i] = (hit && tmax >= fmaxf(tmin, 0.0f)) ? 1 : 0;
}

// Eval-mode refinement of the box test, exact by construction: a ray that stays further than the outlier radius (0.1,
// deformer.py:49) from every vertex between `near` and its far end has only outlier samples, i.e. sdf = 4 on all of them
// (multiply.py:142-143); if moreover alpha = 1 - exp(-sigma(4) (far - near)) is exactly 0 in fp32 (it is for every beta
// below ~0.25: sigma(4) = e^(-4/beta) / (2 beta)) the ray's weights are exactly 0, its transmittance exactly 1, and its
// pixel is the background's -- bit for bit what a ray outside the box gets, and its beta converges in the first sampler
// iteration without touching its group's vote.  Such rays are dropped before they reach the sampler.  The test is
// conservative: the vertex set is covered by the cluster spheres (cbound), inflated by the radius plus a margin for the
// fp32 distance evaluation of the search kernels.
__global__ void k_ray_near_body(const float* __restrict__ dirs, const float* __restrict__ P, const float* __restrict__ cbound,
                                const float* __restrict__ far, const float* __restrict__ beta_p, float near_, int n,
                                int* __restrict__ flag) {
    __shared__ float4 cb[NC];
    for (int c = threadIdx.x; c < NC; c += blockDim.x) cb[c] = ((const float4*)cbound)[c];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const float tf = far[i];
    if (mp::alpha_of(4.0f, *beta_p, tf - near_) != 0.0f) return;   // outliers would still weigh in: keep the ray
    const float ox = P[3], oy = P[7], oz = P[11];
    const float dx = dirs[3 * i], dy = dirs[3 * i + 1], dz = dirs[3 * i + 2];
    bool near_body = false;
    for (int c = 0; c < NC && !near_body; ++c) {
        const float4 b = cb[c];
        const float ex = b.x - ox, ey = b.y - oy, ez = b.z - oz;
        const float t = fminf(fmaxf(ex * dx + ey * dy + ez * dz, near_), tf);   // closest approach inside [near, far]
        const float qx = ex - t * dx, qy = ey - t * dy, qz = ez - t * dz;
        const float reach = b.w + 0.1005f;
        near_body = qx * qx + qy * qy + qz * qz <= reach * reach;
    }
    if (!near_body) flag[i] = 0;
}

// a convergence group without any hit gets its first ray (multiply.py:262-263 applied per group)
__global__ __launch_bounds__(256) void k_group_fallback(int* __restrict__ flag, int n, int group_size) {
    __shared__ int any;
    const int g0 = blockIdx.x * group_size;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    int a = 0;
    for (int i = g0 + threadIdx.x; i < min(n, g0 + group_size); i += 256) a |= flag[i];
    if (a) any = 1;
    __syncthreads();
    if (threadIdx.x == 0 && !any) flag[g0] = 1;
}

constexpr int SCAN_BLOCK = 1024;
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_blocks(const int* __restrict__ flag, int n, int* __restrict__ bsum) {
    __shared__ int sh[SCAN_BLOCK / 64];
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < n ? flag[i] : 0;
    const int c = __popcll(__ballot(f != 0));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < SCAN_BLOCK / 64; ++w) s += sh[w];
        bsum[blockIdx.x] = s;
    }
}
__global__ void k_scan_top(int* __restrict__ bsum, int nb, int* __restrict__ total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int s = 0;
        for (int b = 0; b < nb; ++b) { const int c = bsum[b]; bsum[b] = s; s += c; }
        *total = s;
    }
}
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_scatter(const int* __restrict__ flag, int n,
                                                             const int* __restrict__ bsum, int* __restrict__ hit_index,
                                                             int* __restrict__ inv_index) {
    __shared__ int sh[SCAN_BLOCK / 64];
    const int i = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const int f = i < n ? flag[i] : 0;
    const unsigned long long m = __ballot(f != 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = __popcll(m);
    __syncthreads();
    int base = bsum[blockIdx.x];
    for (int w = 0; w < wave; ++w) base += sh[w];
    const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
    if (i < n) {
        inv_index[i] = f ? pos : -1;
        if (f) hit_index[pos] = i;
    }
}
}  // namespace

static int ray_cull(const float* dirs, const float* pose, const float* obb, const float* cbound, const float* far,
                    const float* beta, float near_, int n_rays, int group_size, int* hit_index, int* hit_count, int* inv_index,
                    int* scan_tmp, void* stream) {
    if (n_rays <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int* flag = scan_tmp;                 // [n_rays]
    int* bsum = scan_tmp + n_rays;        // [nb]
    const int nb = (n_rays + SCAN_BLOCK - 1) / SCAN_BLOCK;
    if (group_size <= 0) group_size = n_rays;
    hipLaunchKernelGGL(k_ray_box, dim3((n_rays + 255) / 256), dim3(256), 0, st, dirs, pose, obb, n_rays, flag);
    if (cbound)
        hipLaunchKernelGGL(k_ray_near_body, dim3((n_rays + 255) / 256), dim3(256), 0, st, dirs, pose, cbound, far, beta, near_,
                           n_rays, flag);
    hipLaunchKernelGGL(k_group_fallback, dim3((n_rays + group_size - 1) / group_size), dim3(256), 0, st, flag, n_rays,
                       group_size);
    hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(SCAN_BLOCK), 0, st, flag, n_rays, bsum);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(64), 0, st, bsum, nb, hit_count);
    hipLaunchKernelGGL(k_scan_scatter, dim3(nb), dim3(SCAN_BLOCK), 0, st, flag, n_rays, bsum, hit_index, inv_index);
    return (int)hipGetLastError();
}

extern "C" int mp_ray_cull(const float* dirs, const float* pose, const float* obb, int n_rays, int group_size,
                           int* hit_index, int* hit_count, int* inv_index, int* scan_tmp, void* stream) {
    return ray_cull(dirs, pose, obb, nullptr, nullptr, nullptr, 0.0f, n_rays, group_size, hit_index, hit_count, inv_index,
                    scan_tmp, stream);
}

extern "C" int mp_ray_cull_near(const float* dirs, const float* pose, const float* obb, const float* cbound, const float* far,
                                const float* beta, float near_, int n_rays, int group_size, int* hit_index, int* hit_count,
                                int* inv_index, int* scan_tmp, void* stream) {
    if (!cbound || !far || !beta) return -1;
    return ray_cull(dirs, pose, obb, cbound, far, beta, near_, n_rays, group_size, hit_index, hit_count, inv_index, scan_tmp,
                    stream);
}

namespace {
__global__ void k_hits_from_index(const int* __restrict__ hit_index, int n_hit, int n_rays, int* __restrict__ hit_count,
                                  int* __restrict__ inv_index, int phase) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (phase == 0) {
        if (i < n_rays) inv_index[i] = -1;
        if (i == 0) *hit_count = n_hit;
    } else if (i < n_hit) {
        inv_index[hit_index[i]] = i;
    }
}
}  // namespace

extern "C" int mp_ray_hits_from_index(const int* hit_index, int n_hit, int n_rays, int* hit_count, int* inv_index,
                                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_hits_from_index, dim3((n_rays + 255) / 256), dim3(256), 0, st, hit_index, n_hit, n_rays,
                       hit_count, inv_index, 0);
    if (n_hit > 0)
        hipLaunchKernelGGL(k_hits_from_index, dim3((n_hit + 255) / 256), dim3(256), 0, st, hit_index, n_hit, n_rays,
                           hit_count, inv_index, 1);
    return (int)hipGetLastError();
}
