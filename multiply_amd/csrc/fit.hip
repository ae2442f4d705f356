// Fitting an SDF network to a closed triangle mesh (multiply_amd/smpl_init.py): the producer of one iteration's training points and
// the objective with its adjoints.  The reference warm-starts its foreground networks from such a fit (multiply.py:101-108) but
// ships neither the file nor the recipe, so the objective is the published one of implicit geometric regularisation (Gropp et al.,
// ICML 2020): the network vanishes on the surface, its gradient equals the normal there, it equals the exact signed distance in
// the volume, and its gradient has unit length everywhere.
//   k_fit_area_cdf  face areas, unit normals and the inclusive area CDF: ONE workgroup walks the faces in tiles of 1024 with a
//                   wave scan (shuffles) + 16 wave totals in LDS, all sums in double and in a fixed order.  Latency-bound, once per fit.
//   k_fit_sample    surface points (face by binary search in the CDF, barycentrics by the square-root map) and volume points
//                   (near-surface copies + box-uniform).  The [n][3] outputs are staged in LDS (stride 3 words: conflict-free on
//                   the 64 banks) and stored as contiguous rows of 768 floats per workgroup.  Latency-bound (the dependent CDF probes).
//   k_fit_loss      the four means and the gradient of their weighted sum in one launch; the gradients need only the set sizes, so
//                   they are elementwise, and the terms are per-thread partials -> wave shuffles -> 16 LDS values summed in order by
//                   every thread.  One workgroup like k_loss_fused: 28 B in + 16 B out per point, latency-bound at 16 k points.
// Entry points: include/multiply_hip.h mp_fit_area_cdf / mp_fit_sample / mp_fit_loss.
#include <hip/hip_runtime.h>
#include "../../include/multiply_hip.h"

namespace {

constexpr int CT = 1024, ST = 256, LT = 1024;
constexpr float TINY = 1e-12f;

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// area (0 for a degenerate face) and unit normal of triangle f
__device__ __forceinline__ float face_area_normal(const float* __restrict__ fv, int f, float* n) {
    const float* p = fv + (size_t)f * 9;
    const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float l = sqrtf(cx * cx + cy * cy + cz * cz);
    if (!(l >= TINY)) { n[0] = n[1] = n[2] = 0.0f; return 0.0f; }
    n[0] = cx / l; n[1] = cy / l; n[2] = cz / l;
    return 0.5f * l;
}

// inclusive sums of one value per thread over the workgroup, in double: returns this thread's prefix and the workgroup total
__device__ __forceinline__ double block_incl_scan(double v, double* sh, double& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    __syncthreads();                       // the previous tile's readers are done with sh
    if (lane == 63) sh[w] = v;
    __syncthreads();
    double base = 0.0, tot = 0.0;
    for (int i = 0; i < CT / 64; ++i) {    // every lane of a wave reads the same word: a broadcast
        if (i < w) base += sh[i];
        tot += sh[i];
    }
    total = tot;
    return base + v;
}

__global__ __launch_bounds__(CT) void k_fit_area_cdf(const float* __restrict__ fv, int F, float* __restrict__ area,
                                                     float* __restrict__ normal, float* __restrict__ cdf) {
    __shared__ double sh[CT / 64];
    const int t = threadIdx.x;
    double carry = 0.0, tile;
    for (int f0 = 0; f0 < F; f0 += CT) {   // pass 1: areas, normals, the total
        const int f = f0 + t;
        float a = 0.0f;
        if (f < F) {
            float n[3];
            a = face_area_normal(fv, f, n);
            area[f] = a;
            normal[3 * (size_t)f] = n[0]; normal[3 * (size_t)f + 1] = n[1]; normal[3 * (size_t)f + 2] = n[2];
        }
        block_incl_scan((double)a, sh, tile);
        carry += tile;
    }
    const double total = carry;
    carry = 0.0;
    for (int f0 = 0; f0 < F; f0 += CT) {   // pass 2: every thread re-reads the areas it wrote itself
        const int f = f0 + t;
        const double incl = block_incl_scan(f < F ? (double)area[f] : 0.0, sh, tile);
        if (f < F) cdf[f] = total > 0.0 ? (float)((carry + incl) / total) : 0.0f;
        carry += tile;
    }
}

// surface point from three uniforms; returns the face
__device__ __forceinline__ int surface_point(const float* __restrict__ fv, const float* __restrict__ cdf, int F,
                                             const float* __restrict__ u, float* p) {
    const float u0 = u[0], r = sqrtf(u[1]), u2 = u[2];
    int lo = 0, hi = F - 1;
    while (lo < hi) {                      // first face whose inclusive CDF exceeds u0 (a zero-area face never is)
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > u0) hi = mid; else lo = mid + 1;
    }
    const float* q = fv + (size_t)lo * 9;
    const float b0 = 1.0f - r, b1 = r * (1.0f - u2), b2 = r * u2;
    for (int c = 0; c < 3; ++c) p[c] = b0 * q[c] + b1 * q[3 + c] + b2 * q[6 + c];
    return lo;
}

// rows [row0, row0 + rows) of an [n][3] array from the workgroup's LDS stage: contiguous, coalesced
__device__ __forceinline__ void store_rows3(const float* st, float* __restrict__ out, int row0, int rows) {
    for (int k = threadIdx.x; k < rows * 3; k += ST) out[(size_t)row0 * 3 + k] = st[k];
}

__global__ __launch_bounds__(ST) void k_fit_sample(const float* __restrict__ fv, const float* __restrict__ normal,
                                                   const float* __restrict__ cdf, int F, const float* __restrict__ u_surf, int n_s,
                                                   const float* __restrict__ z_near, int n_near, float sigma,
                                                   const float* __restrict__ u_box, const float* __restrict__ box, int n_v,
                                                   float* __restrict__ surf_pts, float* __restrict__ surf_nrm,
                                                   int* __restrict__ face_id, float* __restrict__ vol_pts) {
    __shared__ float sp[ST * 3], sn[ST * 3];
    const int t = threadIdx.x, nbs = (n_s + ST - 1) / ST;
    if ((int)blockIdx.x < nbs) {           // a workgroup of surface points
        const int row0 = blockIdx.x * ST, i = row0 + t, rows = min(ST, n_s - row0);
        if (i < n_s) {
            float p[3];
            const int f = surface_point(fv, cdf, F, u_surf + 3 * (size_t)i, p);
            face_id[i] = f;
            for (int c = 0; c < 3; ++c) { sp[3 * t + c] = p[c]; sn[3 * t + c] = normal[3 * (size_t)f + c]; }
        }
        __syncthreads();
        store_rows3(sp, surf_pts, row0, rows);
        store_rows3(sn, surf_nrm, row0, rows);
    } else {                               // a workgroup of volume points
        const int row0 = ((int)blockIdx.x - nbs) * ST, j = row0 + t, rows = min(ST, n_v - row0);
        if (j < n_v) {
            float p[3];
            if (j < n_near) {              // the same arithmetic as the surface workgroups: bit-identical copies
                surface_point(fv, cdf, F, u_surf + 3 * (size_t)(j % n_s), p);
                for (int c = 0; c < 3; ++c) p[c] += sigma * z_near[3 * (size_t)j + c];
            } else {
                const float* u = u_box + 3 * (size_t)(j - n_near);
                for (int c = 0; c < 3; ++c) p[c] = box[c] + u[c] * (box[3 + c] - box[c]);
            }
            for (int c = 0; c < 3; ++c) sp[3 * t + c] = p[c];
        }
        __syncthreads();
        store_rows3(sp, vol_pts, row0, rows);
    }
}

__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    for (int i = 0; i < LT / 64; ++i) t += sh[i];
    return t;
}

__global__ __launch_bounds__(LT) void k_fit_loss(const float* __restrict__ sdf, const float* __restrict__ grad,
                                                 const float* __restrict__ normals, const float* __restrict__ dist, int n_s, int n_v,
                                                 float w_s, float w_n, float w_d, float w_e, float tau, float* __restrict__ terms,
                                                 float* __restrict__ d_sdf, float* __restrict__ d_grad) {
    __shared__ float sh[LT / 64];
    const int n = n_s + n_v;
    const float inv_s = n_s > 0 ? 1.0f / (float)n_s : 0.0f, inv_v = n_v > 0 ? 1.0f / (float)n_v : 0.0f;
    const float inv_n = n > 0 ? 1.0f / (float)n : 0.0f;
    float s_surf = 0.0f, s_nrm = 0.0f, s_dist = 0.0f, s_eik = 0.0f;
    for (int i = threadIdx.x; i < n; i += LT) {
        const float f = sdf[i], gx = grad[3 * (size_t)i], gy = grad[3 * (size_t)i + 1], gz = grad[3 * (size_t)i + 2];
        const float gn = sqrtf(gx * gx + gy * gy + gz * gz);
        s_eik += (gn - 1.0f) * (gn - 1.0f);
        const float ke = gn >= TINY ? w_e * 2.0f * (gn - 1.0f) * inv_n / gn : 0.0f;
        float dx = ke * gx, dy = ke * gy, dz = ke * gz, df;
        if (i < n_s) {
            s_surf += fabsf(f);
            df = w_s * sgn(f) * inv_s;
            const float rx = gx - normals[3 * (size_t)i], ry = gy - normals[3 * (size_t)i + 1], rz = gz - normals[3 * (size_t)i + 2];
            const float rn = sqrtf(rx * rx + ry * ry + rz * rz);
            s_nrm += rn;
            const float kn = rn >= TINY ? w_n * inv_s / rn : 0.0f;
            dx += kn * rx; dy += kn * ry; dz += kn * rz;
        } else {
            const float d = dist[i - n_s];
            const bool trunc = tau > 0.0f;
            const float cf = trunc ? fminf(fmaxf(f, -tau), tau) : f, cd = trunc ? fminf(fmaxf(d, -tau), tau) : d;
            s_dist += fabsf(cf - cd);
            const bool pass = !trunc || (f >= -tau && f <= tau);         // the clamp passes the gradient inside its range
            df = pass ? w_d * sgn(cf - cd) * inv_v : 0.0f;
        }
        d_sdf[i] = df;
        d_grad[3 * (size_t)i] = dx; d_grad[3 * (size_t)i + 1] = dy; d_grad[3 * (size_t)i + 2] = dz;
    }
    s_surf = block_sum(s_surf, sh);
    s_nrm = block_sum(s_nrm, sh);
    s_dist = block_sum(s_dist, sh);
    s_eik = block_sum(s_eik, sh);
    if (threadIdx.x == 0) {
        const float t1 = s_surf * inv_s, t2 = s_nrm * inv_s, t3 = s_dist * inv_v, t4 = s_eik * inv_n;
        terms[0] = w_s * t1 + w_n * t2 + w_d * t3 + w_e * t4;
        terms[1] = t1; terms[2] = t2; terms[3] = t3; terms[4] = t4;
    }
}

}  // namespace

extern "C" int mp_fit_area_cdf(const float* face_verts, int n_faces, float* area, float* normal, float* cdf, void* stream) {
    if (n_faces <= 0 || !face_verts || !area || !normal || !cdf) return -1;
    hipLaunchKernelGGL(k_fit_area_cdf, dim3(1), dim3(CT), 0, (hipStream_t)stream, face_verts, n_faces, area, normal, cdf);
    return (int)hipGetLastError();
}

extern "C" int mp_fit_sample(const float* face_verts, const float* normal, const float* cdf, int n_faces, const float* u_surf,
                             int n_s, const float* z_near, int n_near, float sigma_local, const float* u_box, const float* box,
                             int n_v, float* surf_pts, float* surf_nrm, int* face_id, float* vol_pts, void* stream) {
    if (n_faces <= 0 || n_s < 0 || n_v < 0 || n_near < 0 || n_near > n_v || (n_near > 0 && n_s == 0)) return -1;
    if (!face_verts || !normal || !cdf) return -1;
    if (n_s > 0 && (!u_surf || !surf_pts || !surf_nrm || !face_id)) return -1;
    if (n_v > 0 && !vol_pts) return -1;
    if (n_near > 0 && !z_near) return -1;
    if (n_v > n_near && (!u_box || !box)) return -1;
    const int blocks = (n_s + ST - 1) / ST + (n_v + ST - 1) / ST;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(k_fit_sample, dim3(blocks), dim3(ST), 0, (hipStream_t)stream, face_verts, normal, cdf, n_faces, u_surf, n_s,
                       z_near, n_near, sigma_local, u_box, box, n_v, surf_pts, surf_nrm, face_id, vol_pts);
    return (int)hipGetLastError();
}

extern "C" int mp_fit_loss(const float* sdf, const float* grad, const float* normals, const float* dist, int n_s, int n_v,
                           float w_surface, float w_normal, float w_distance, float w_eikonal, float truncation, float* terms,
                           float* d_sdf, float* d_grad, void* stream) {
    if (n_s < 0 || n_v < 0 || !terms) return -1;
    if (n_s + n_v > 0 && (!sdf || !grad || !d_sdf || !d_grad)) return -1;
    if ((n_s > 0 && !normals) || (n_v > 0 && !dist)) return -1;
    hipLaunchKernelGGL(k_fit_loss, dim3(1), dim3(LT), 0, (hipStream_t)stream, sdf, grad, normals, dist, n_s, n_v, w_surface,
                       w_normal, w_distance, w_eikonal, truncation, terms, d_sdf, d_grad);
    return (int)hipGetLastError();
}
