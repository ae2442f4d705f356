// Small device helpers shared by the kernels: density, the wave / workgroup reductions and the wave-level LDS fence, the per-device LDS attribute.
#pragma once
#include <hip/hip_runtime.h>

namespace mp {

// LaplaceDensity.density_func (reference code/lib/model/density.py:20-29):
//   sigma = (1/beta) * (0.5 + 0.5 * sign(sdf) * expm1(-|sdf| / beta))
__device__ __forceinline__ float laplace_density(float sdf, float beta) {
    const float sgn = sdf > 0.0f ? 1.0f : (sdf < 0.0f ? -1.0f : 0.0f);
    return (1.0f / beta) * (0.5f + 0.5f * sgn * expm1f(-fabsf(sdf) / beta));
}

// its adjoint: dsdf = d sigma / d sdf, dbeta = d sigma / d beta
__device__ __forceinline__ void laplace_density_adjoint(float s, float beta, float& dsdf, float& dbeta) {
    const float eab = expf(-fabsf(s) / beta);
    dsdf = -(0.5f / (beta * beta)) * eab;
    if (s > 0.f) dbeta = (0.5f / (beta * beta)) * eab * (s / beta - 1.0f);
    else if (s < 0.f) dbeta = -1.0f / (beta * beta) + (0.5f / (beta * beta)) * eab * (1.0f + s / beta);
    else dbeta = -0.5f / (beta * beta);
}

// alpha of one sample exactly as the compositing kernel computes it (multiply.py:455 via nerfacc):
//   alpha = 1 - exp(-sigma * dt)
__device__ __forceinline__ float alpha_of(float sdf, float beta, float dt) {
    return 1.0f - expf(-(laplace_density(sdf, beta) * dt));
}

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wmin(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
// orders this wave's LDS traffic: writes by any lane before, reads by any lane after (LDS the wave shares with no other wave)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// block-wide sum for blockDim.x = 256 (4 waves)
__device__ __forceinline__ float block_sum256(float v, float* sh) {
    v = wsum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
// exclusive prefix sum across the 64 lanes of a wave; `total` receives the wave sum
__device__ __forceinline__ float wave_excl_scan(float v, float& total) {
    float incl = v;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float n = __shfl_up(incl, o);
        if (lane >= o) incl += n;
    }
    total = __shfl(incl, 63);
    return incl - v;
}

// Adjoint of one point's Fourier features (embedders.py layout: x, then per octave k  sin(2^k x), cos(2^k x), D columns each)
// w.r.t. component a of the point: dv(c) = adjoint of column c of the value row; fwd: dt(c) = adjoint of column c of
// component a's tangent row (1, f cos(f x_a), -f sin(f x_a)).  THE arithmetic of k_pe_bwd (train.hip) and of k_tf_sdf_dx
// (tfuse.hip): both paths to the points' adjoint evaluate the same expression in the same order.
template <int D, class DV, class DT>
__device__ __forceinline__ float pe_adjoint(float xa, int a, int L, bool fwd, DV dv, DT dt) {
    float acc = dv(a);
    for (int k = 0; k < L; ++k) {
        const float f = (float)(1 << k);
        float sn, cs;
        sincosf(xa * f, &sn, &cs);
        const int cs_ = D + 2 * D * k + a, cc_ = cs_ + D;
        acc += f * (cs * dv(cs_) - sn * dv(cc_));
        if (fwd) acc -= f * f * (sn * dt(cs_) + cs * dt(cc_));
    }
    return acc;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute: a `static int once = hipFuncSetAttribute(...)` covers
// only the device that is current at the first call.  MP_LDS_ATTR(kernel, bytes) sets it once per (call site, device ordinal)
// and makes the enclosing entry point return the HIP error code if the runtime refuses.
inline int lds_attr(const void* kernel, int bytes, unsigned long long& done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (dev < 64 && ((done_mask >> dev) & 1ull)) return 0;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    if (dev < 64) done_mask |= 1ull << dev;
    return 0;
}
#define MP_LDS_ATTR(kernel, bytes)                                                    \
    do {                                                                              \
        static unsigned long long mp_lds_done_ = 0;                                   \
        const int mp_lds_rc_ = mp::lds_attr((const void*)(kernel), (bytes), mp_lds_done_); \
        if (mp_lds_rc_) return mp_lds_rc_;                                            \
    } while (0)

}  // namespace mp
