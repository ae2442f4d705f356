// The optimiser of the training loop (multiply_amd/trainer.py DeviceAdam): torch.optim.Adam's single-tensor step (no weight decay,
// no amsgrad) for EVERY parameter tensor of an optimiser in one launch.  Entry point: include/multiply_hip.h (mp_adam_multi).
//
// The tensors are described by a device array of MpAdamDesc records; the blocks of all tensors are concatenated in one grid
// (block0 = first block of a tensor, ascending; a block finds its tensor by binary search, as k_wn_fwd_multi does).  A tensor
// owns at most n_block blocks and strides over the rest of its elements.  Learning rates (one per group) and the skip flag are
// read from device memory: a schedule change or a NaN loss needs neither a table rebuild nor a host round trip.
//
// Step counts: every tensor has its own count t (a device float, as in torch's state dict).  k_adam_multi only READS the counts
// (all blocks of a tensor see the same t and use t + 1); the counts of the active tensors are incremented by k_adam_count, a
// trailing n_desc-thread launch on the same stream.  No launch reads a count it writes.
#include <hip/hip_runtime.h>
#include "../../include/multiply_hip.h"

namespace {

constexpr int TB = 256;

struct AdamK {
    float w1;         // 1 - beta1
    float beta2;
    float w2;         // 1 - beta2
    float eps;
    float step_size;  // lr / (1 - beta1^t)
    float bc2;        // sqrt(1 - beta2^t)
};

// torch.optim.Adam (single tensor form) on one element; explicit fused multiply-adds: the rounding of a step is spelled out, not
// left to the compiler's contraction (the same statements as csrc/keypoint_fit.hip k_kp_fit)
__device__ __forceinline__ void adam1(const AdamK& k, float& p, float g, float& m, float& v) {
    m = fmaf(g - m, k.w1, m);                        // exp_avg.lerp_(grad, 1 - beta1)
    v = fmaf(v, k.beta2, (k.w2 * g) * g);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / k.bc2 + k.eps;
    p = fmaf(-k.step_size, m / denom, p);            // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__device__ __forceinline__ void adam_scalar(const AdamK& k, const MpAdamDesc& D, long long i) {
    float p = D.p[i], m = D.m[i], v = D.v[i];
    adam1(k, p, D.g[i], m, v);
    D.p[i] = p; D.m[i] = m; D.v[i] = v;
}

__device__ __forceinline__ int adam_find(const MpAdamDesc* __restrict__ d, int n, int block) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (d[mid].block0 <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(TB) void k_adam_multi(const MpAdamDesc* __restrict__ descs, int n_desc, const float* __restrict__ lr,
                                                   const unsigned char* __restrict__ skip, double beta1, double beta2, float eps) {
    if (skip && *skip) return;
    const MpAdamDesc D = descs[adam_find(descs, n_desc, blockIdx.x)];
    if (!D.g || D.n <= 0) return;
    // the bias corrections in double from the tensor's own count, as the python scalars of torch's step are
    const double t = (double)*D.step + 1.0;
    AdamK k;
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = eps;
    k.step_size = (float)((double)lr[D.group] / (1.0 - pow(beta1, t)));
    k.bc2 = (float)sqrt(1.0 - pow(beta2, t));
    const long long b = (int)blockIdx.x - D.block0, nb = D.n_block > 0 ? D.n_block : 1;
    if (b >= nb) return;                              // a grid larger than the table's block ranges: nothing to do
    const long long tid = b * TB + threadIdx.x, stride = nb * TB;
    if (D.mode == MP_ADAM_SCALAR) {
        for (long long i = tid; i < D.n; i += stride) adam_scalar(k, D, i);
        return;
    }
    // 16-byte accesses: p, m and v share their offset within 16 bytes (MP_ADAM_VEC: g too; MP_ADAM_VEC_G4: g is read by dwords)
    long long head = (long long)(((16u - (unsigned)((unsigned long long)D.p & 15u)) & 15u) >> 2);
    if (head > D.n) head = D.n;
    const long long nvec = (D.n - head) >> 2, tail0 = head + 4 * nvec;
    float4* p4 = (float4*)(D.p + head);
    float4* m4 = (float4*)(D.m + head);
    float4* v4 = (float4*)(D.v + head);
    const float* g1 = D.g + head;
    for (long long i = tid; i < nvec; i += stride) {
        float4 p = p4[i], m = m4[i], v = v4[i], g;
        if (D.mode == MP_ADAM_VEC) g = ((const float4*)g1)[i];
        else { g.x = g1[4 * i]; g.y = g1[4 * i + 1]; g.z = g1[4 * i + 2]; g.w = g1[4 * i + 3]; }
        adam1(k, p.x, g.x, m.x, v.x);
        adam1(k, p.y, g.y, m.y, v.y);
        adam1(k, p.z, g.z, m.z, v.z);
        adam1(k, p.w, g.w, m.w, v.w);
        p4[i] = p; m4[i] = m; v4[i] = v;
    }
    if (b == 0) {                                     // scalar head and tail: at most 3 elements each
        if ((long long)threadIdx.x < head) adam_scalar(k, D, threadIdx.x);
        const long long j = tail0 + ((long long)threadIdx.x - 8);
        if (threadIdx.x >= 8 && j < D.n) adam_scalar(k, D, j);
    }
}

__global__ void k_adam_count(const MpAdamDesc* __restrict__ descs, int n_desc, const unsigned char* __restrict__ skip) {
    if (skip && *skip) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_desc && descs[i].g && descs[i].n > 0) *descs[i].step += 1.0f;
}

}  // namespace

extern "C" int mp_adam_multi(const MpAdamDesc* descs, int n_desc, int total_blocks, const float* lr, const unsigned char* skip,
                             double beta1, double beta2, double eps, void* stream) {
    if (n_desc < 0 || total_blocks < 0) return -1;
    if (n_desc == 0 || total_blocks == 0) return 0;
    if (!descs || !lr) return -1;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0)) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_adam_multi, dim3(total_blocks), dim3(TB), 0, st, descs, n_desc, lr, skip, beta1, beta2, (float)eps);
    hipLaunchKernelGGL(k_adam_count, dim3((n_desc + TB - 1) / TB), dim3(TB), 0, st, descs, n_desc, skip);
    return (int)hipGetLastError();
}
