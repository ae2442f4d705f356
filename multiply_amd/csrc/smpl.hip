// SMPL body model: shape and pose blend shapes, kinematic chain, linear blend skinning (mp_smpl_pose; N rows in two launches:
// mp_smpl_pose_batch), the adjoint of the posed vertices (mp_smpl_verts_bwd) and of the chain (mp_smpl_pose_bwd, mp_smpl_pose_bwd_lbs).
// Entry points and the reference code they replace: include/multiply_hip.h.
#include <hip/hip_runtime.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "smpl_chain.hpp"

namespace {
constexpr int V = MP_SMPL_V, NJ = MP_SMPL_J;

// ------------------------------------------------------------------------------------------------ SMPL (lbs.py)
// work layout (floats): v_shaped [3V] | J [72] | A [24*16] | pose_feature [207]
constexpr int W_VS = 0, W_J = 3 * V, W_A = W_J + 72 + 8, W_PF = W_A + NJ * 16;

__global__ void k_smpl_shape(const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                             const float* __restrict__ params, float* __restrict__ work) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // over V*3
    if (i >= 3 * V) return;
    const float* betas = params + 76;
    float acc = 0.0f;
#pragma unroll
    for (int l = 0; l < 10; ++l) acc += betas[l] * shapedirs[(size_t)i * 10 + l];  // blend_shapes, lbs.py:252-273
    work[W_VS + i] = v_template[i] + acc;
}

__global__ __launch_bounds__(256) void k_smpl_joints(const float* __restrict__ j_regressor, float* __restrict__ work) {
    __shared__ float sh[4];
    const int j = blockIdx.x;  // joint
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = threadIdx.x; i < V; i += 256) {  // vertices2joints, lbs.py:232-249
        const float w = j_regressor[(size_t)j * V + i];
        a0 += w * work[W_VS + 3 * i];
        a1 += w * work[W_VS + 3 * i + 1];
        a2 += w * work[W_VS + 3 * i + 2];
    }
    a0 = mp::block_sum256(a0, sh);
    a1 = mp::block_sum256(a1, sh);
    a2 = mp::block_sum256(a2, sh);
    if (threadIdx.x == 0) { work[W_J + 3 * j] = a0; work[W_J + 3 * j + 1] = a1; work[W_J + 3 * j + 2] = a2; }
}

__device__ void mat4_mul(const float* a, const float* b, float* c) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j];
            c[4 * i + j] = s;
        }
}

__global__ __launch_bounds__(64) void k_smpl_chain(const int* __restrict__ parents, const float* __restrict__ params,
                                                   const float* __restrict__ tfs_c_inv, float* __restrict__ work,
                                                   float* __restrict__ tfs, float* __restrict__ joints) {
    __shared__ float R[NJ][9];
    __shared__ float G[NJ][16];
    const int t = threadIdx.x;
    const float scale = params[0];
    const float* transl = params + 1;
    const float* thetas = params + 4;
    const float* J = work + W_J;
    if (t < NJ) {  // batch_rodrigues, lbs.py:276-307
        const float rx0 = thetas[3 * t], ry0 = thetas[3 * t + 1], rz0 = thetas[3 * t + 2];
        const float ax = rx0 + 1e-8f, ay = ry0 + 1e-8f, az = rz0 + 1e-8f;
        const float angle = sqrtf(ax * ax + ay * ay + az * az);
        const float rx = rx0 / angle, ry = ry0 / angle, rz = rz0 / angle;
        float s, c;
        sincosf(angle, &s, &c);
        const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
        float KK[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                float a = 0.f;
                for (int k = 0; k < 3; ++k) a += K[3 * i + k] * K[3 * k + j];
                KK[3 * i + j] = a;
            }
        for (int i = 0; i < 9; ++i) R[t][i] = ((i % 4 == 0) ? 1.0f : 0.0f) + s * K[i] + (1.0f - c) * KK[i];
    }
    __syncthreads();
    // pose_feature = (R[1:] - I).flatten (lbs.py:199)
    for (int i = t; i < 207; i += 64) {
        const int j = i / 9 + 1, e = i % 9;
        work[W_PF + i] = R[j][e] - ((e % 4 == 0) ? 1.0f : 0.0f);
    }
    if (t == 0) {  // batch_rigid_transform, lbs.py:323-377 (24 tiny sequential 4x4 products)
        for (int j = 0; j < NJ; ++j) {
            const int p = parents[j];
            float rel[3];
            for (int a = 0; a < 3; ++a) rel[a] = J[3 * j + a] - (j > 0 ? J[3 * p + a] : 0.0f);
            float tm[16];
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) tm[4 * a + b] = R[j][3 * a + b];
                tm[4 * a + 3] = rel[a];
            }
            tm[12] = tm[13] = tm[14] = 0.f;
            tm[15] = 1.f;
            if (j == 0) for (int i = 0; i < 16; ++i) G[0][i] = tm[i];
            else mat4_mul(G[p], tm, G[j]);
        }
    }
    __syncthreads();
    if (t < NJ) {
        float A[16];
        for (int i = 0; i < 16; ++i) A[i] = G[t][i];
        // rel_transforms = G - pad(G @ [J;0])  (lbs.py:372-375)
        for (int a = 0; a < 4; ++a) {
            float s = 0.f;
            for (int k = 0; k < 3; ++k) s += G[t][4 * a + k] * J[3 * t + k];
            A[4 * a + 3] -= s;
        }
        for (int i = 0; i < 16; ++i) work[W_A + 16 * t + i] = A[i];
        // SMPLServer.forward scaling (smpl.py:80-91)
        float tf[16];
        for (int i = 0; i < 16; ++i) tf[i] = A[i];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 4; ++b) tf[4 * a + b] *= scale;
            tf[4 * a + 3] += transl[a] * scale;
        }
        if (tfs_c_inv) {
            float o[16];
            mat4_mul(tf, tfs_c_inv + 16 * t, o);
            for (int i = 0; i < 16; ++i) tfs[16 * t + i] = o[i];
        } else {
            for (int i = 0; i < 16; ++i) tfs[16 * t + i] = tf[i];
        }
        for (int a = 0; a < 3; ++a) joints[3 * t + a] = G[t][4 * a + 3] * scale + transl[a] * scale;
    }
}

__global__ __launch_bounds__(256) void k_smpl_verts(const float* __restrict__ posedirs,
                                                    const float* __restrict__ lbs_weights,
                                                    const float* __restrict__ params, const float* __restrict__ work,
                                                    float* __restrict__ verts) {
    __shared__ float pf[207];
    __shared__ float A[NJ * 16];
    for (int i = threadIdx.x; i < 207; i += 256) pf[i] = work[W_PF + i];
    for (int i = threadIdx.x; i < NJ * 16; i += 256) A[i] = work[W_A + i];
    __syncthreads();
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float acc = 0.f;
        for (int q = 0; q < 207; ++q) acc += pf[q] * posedirs[(size_t)q * (3 * V) + 3 * v + k];  // lbs.py:201-202
        p[k] = acc + work[W_VS + 3 * v + k];
    }
    float T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
    for (int j = 0; j < NJ; ++j) {  // lbs.py:217-221
        const float w = lbs_weights[(size_t)v * NJ + j];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] += w * A[16 * j + i];
    }
    const float scale = params[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float x = T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3];
        verts[3 * v + a] = x * scale + params[1 + a] * scale;  // smpl.py:77-78
    }
}
}  // namespace

extern "C" int mp_smpl_pose(const float* v_template, const float* shapedirs, const float* posedirs,
                            const float* j_regressor, const float* lbs_weights, const int* parents, const float* params,
                            const float* tfs_c_inv, float* verts, float* tfs, float* joints, float* work, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smpl_shape, dim3((3 * V + 255) / 256), dim3(256), 0, st, v_template, shapedirs, params, work);
    hipLaunchKernelGGL(k_smpl_joints, dim3(NJ), dim3(256), 0, st, j_regressor, work);
    hipLaunchKernelGGL(k_smpl_chain, dim3(1), dim3(64), 0, st, parents, params, tfs_c_inv, work, tfs, joints);
    hipLaunchKernelGGL(k_smpl_verts, dim3((V + 255) / 256), dim3(256), 0, st, posedirs, lbs_weights, params, work, verts);
    return (int)hipGetLastError();
}

namespace {
// ---- N parameter rows in two launches (mp_smpl_pose_batch), forward only.
//   k_smpl_batch_chain  one workgroup per row: the rest joints from v_shaped formed on the fly (per thread the vertices t, t + 256,
//                       ... in order, then block_sum256: k_smpl_shape + k_smpl_joints in one), then smpl_batch_chain_row.  Leaves
//                       J | A | pose feature in the row's work slice.
//   k_smpl_batch_verts  one workgroup per BT_V = 32 vertices: the 207 x 96 tile of posedirs is staged in LDS ONCE and swept over
//                       all rows, BT_ROWS = 16 at a time.  Thread (slot, column) holds its column's v_template and shapedirs in
//                       registers and runs the 207-term sums of the slot's four rows off one LDS read of the tile per term; the
//                       blend and the skinning then go one thread per (row, vertex).
// A row's operations and their order do not depend on N or on where the row stands (rows only share the tile), so a row has the
// same bits alone and in any batch.  No atomics.
constexpr int BW_J = 0, BW_A = 80, BW_PF = BW_A + NJ * 16, BW_ROW = MP_SMPL_BATCH_ROW_WORK;
constexpr int BT_V = 32, BT_COLS = 3 * BT_V, BT_SLOTS = 4, BT_RB = 4, BT_ROWS = BT_SLOTS * BT_RB, BT_THREADS = BT_SLOTS * BT_COLS;
constexpr int BT_BLOCKS = (V + BT_V - 1) / BT_V, BT_WLD = NJ + 1, BT_PRM = 16;
static_assert(BW_PF + 207 <= BW_ROW && BT_ROWS == MP_SMPL_BATCH_ROWS && BT_THREADS % 64 == 0 && BT_COLS % 2 == 0 && BT_RB == 4,
              "layout of mp_smpl_pose_batch");

// Rodrigues, pose feature, kinematic chain and SMPLServer.forward's scaling of ONE row by the first 24 threads of a workgroup of
// 256 (every thread must call: two barriers).  The statements of k_smpl_chain, written again instead of shared: moving that
// kernel's body into a function changed how the compiler contracts six of its multiply-adds, and mp_smpl_pose keeps its bits.
// J: the row's rest joints (LDS); wA / wPF: where its rest-relative transforms [24][16] and pose feature [207] go; tfs / joints:
// the row's outputs, either may be NULL.
__device__ __forceinline__ void smpl_batch_chain_row(const int* __restrict__ parents, const float* __restrict__ params,
                                                     const float* __restrict__ tfs_c_inv, const float* J, float* __restrict__ wA,
                                                     float* __restrict__ wPF, float* __restrict__ tfs, float* __restrict__ joints,
                                                     float (*R)[9], float (*G)[16]) {
    const int t = threadIdx.x;
    const float scale = params[0];
    const float* transl = params + 1;
    const float* thetas = params + 4;
    if (t < NJ) {  // batch_rodrigues, lbs.py:276-307
        const float rx0 = thetas[3 * t], ry0 = thetas[3 * t + 1], rz0 = thetas[3 * t + 2];
        const float ax = rx0 + 1e-8f, ay = ry0 + 1e-8f, az = rz0 + 1e-8f;
        const float angle = sqrtf(ax * ax + ay * ay + az * az);
        const float rx = rx0 / angle, ry = ry0 / angle, rz = rz0 / angle;
        float s, c;
        sincosf(angle, &s, &c);
        const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
        float KK[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                float a = 0.f;
                for (int k = 0; k < 3; ++k) a += K[3 * i + k] * K[3 * k + j];
                KK[3 * i + j] = a;
            }
        for (int i = 0; i < 9; ++i) R[t][i] = ((i % 4 == 0) ? 1.0f : 0.0f) + s * K[i] + (1.0f - c) * KK[i];
    }
    __syncthreads();
    for (int i = t; i < 207; i += 256) {  // pose_feature = (R[1:] - I).flatten (lbs.py:199)
        const int j = i / 9 + 1, e = i % 9;
        wPF[i] = R[j][e] - ((e % 4 == 0) ? 1.0f : 0.0f);
    }
    if (t == 0) {  // batch_rigid_transform, lbs.py:323-377 (24 tiny sequential 4x4 products)
        for (int j = 0; j < NJ; ++j) {
            const int p = parents[j];
            float rel[3];
            for (int a = 0; a < 3; ++a) rel[a] = J[3 * j + a] - (j > 0 ? J[3 * p + a] : 0.0f);
            float tm[16];
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) tm[4 * a + b] = R[j][3 * a + b];
                tm[4 * a + 3] = rel[a];
            }
            tm[12] = tm[13] = tm[14] = 0.f;
            tm[15] = 1.f;
            if (j == 0) for (int i = 0; i < 16; ++i) G[0][i] = tm[i];
            else mat4_mul(G[p], tm, G[j]);
        }
    }
    __syncthreads();
    if (t < NJ) {
        float A[16];
        for (int i = 0; i < 16; ++i) A[i] = G[t][i];
        for (int a = 0; a < 4; ++a) {  // rel_transforms = G - pad(G @ [J;0])  (lbs.py:372-375)
            float s = 0.f;
            for (int k = 0; k < 3; ++k) s += G[t][4 * a + k] * J[3 * t + k];
            A[4 * a + 3] -= s;
        }
        for (int i = 0; i < 16; ++i) wA[16 * t + i] = A[i];
        float tf[16];  // SMPLServer.forward scaling (smpl.py:80-91)
        for (int i = 0; i < 16; ++i) tf[i] = A[i];
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 4; ++b) tf[4 * a + b] *= scale;
            tf[4 * a + 3] += transl[a] * scale;
        }
        if (tfs && tfs_c_inv) {
            float o[16];
            mat4_mul(tf, tfs_c_inv + 16 * t, o);
            for (int i = 0; i < 16; ++i) tfs[16 * t + i] = o[i];
        } else if (tfs) {
            for (int i = 0; i < 16; ++i) tfs[16 * t + i] = tf[i];
        }
        if (joints)
            for (int a = 0; a < 3; ++a) joints[3 * t + a] = G[t][4 * a + 3] * scale + transl[a] * scale;
    }
}

__global__ __launch_bounds__(256) void k_smpl_batch_chain(const float* __restrict__ v_template,
                                                          const float* __restrict__ shapedirs,
                                                          const float* __restrict__ j_regressor,
                                                          const int* __restrict__ parents, const float* __restrict__ params,
                                                          const float* __restrict__ tfs_c_inv, float* __restrict__ work,
                                                          float* __restrict__ tfs, float* __restrict__ joints) {
    __shared__ float R[NJ][9];
    __shared__ float G[NJ][16];
    __shared__ float Js[3 * NJ], sh[4];
    const int t = threadIdx.x;
    const size_t n = blockIdx.x;
    const float* prm = params + n * 86;
    float* w = work + n * BW_ROW;
    float betas[10], acc[3 * NJ];
#pragma unroll
    for (int l = 0; l < 10; ++l) betas[l] = prm[76 + l];
#pragma unroll
    for (int e = 0; e < 3 * NJ; ++e) acc[e] = 0.f;
    for (int i = t; i < V; i += 256) {
        float vs[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float a = 0.0f;
#pragma unroll
            for (int l = 0; l < 10; ++l) a += betas[l] * shapedirs[(size_t)(3 * i + k) * 10 + l];  // blend_shapes, lbs.py:252-273
            vs[k] = v_template[3 * i + k] + a;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {                              // vertices2joints, lbs.py:232-249
            const float wj = j_regressor[(size_t)j * V + i];
            acc[3 * j] += wj * vs[0];
            acc[3 * j + 1] += wj * vs[1];
            acc[3 * j + 2] += wj * vs[2];
        }
    }
#pragma unroll
    for (int e = 0; e < 3 * NJ; ++e) {
        const float s = mp::block_sum256(acc[e], sh);
        if (t == 0) { Js[e] = s; w[BW_J + e] = s; }
    }
    __syncthreads();
    smpl_batch_chain_row(parents, prm, tfs_c_inv, Js, w + BW_A, w + BW_PF, tfs ? tfs + n * NJ * 16 : nullptr,
                         joints ? joints + n * NJ * 3 : nullptr, R, G);
}

__global__ __launch_bounds__(BT_THREADS) void k_smpl_batch_verts(const float* __restrict__ posedirs,
                                                                 const float* __restrict__ shapedirs,
                                                                 const float* __restrict__ v_template,
                                                                 const float* __restrict__ lbs_weights,
                                                                 const float* __restrict__ params,
                                                                 const float* __restrict__ work, int N,
                                                                 float* __restrict__ verts) {
    __shared__ float P[207 * BT_COLS];
    __shared__ __attribute__((aligned(16))) float pfs[BT_SLOTS * 207 * BT_RB];   // [slot][term][row of the slot]
    __shared__ float As[BT_ROWS * NJ * 12], W[BT_V * BT_WLD], pv[BT_ROWS * BT_COLS], prm[BT_ROWS * BT_PRM];
    const int t = threadIdx.x, v0 = blockIdx.x * BT_V, nv = min(BT_V, V - v0);
    const int slot = t / BT_COLS, c = t % BT_COLS, gc = 3 * v0 + c;
    for (int e = t; e < 207 * (BT_COLS / 2); e += BT_THREADS) {   // the tile, 8-byte loads (3V and the tile's first column are even)
        const int r = e / (BT_COLS / 2), cc = 2 * (e % (BT_COLS / 2)), g = 3 * v0 + cc;
        float2 x = make_float2(0.f, 0.f);
        if (g < 3 * V) x = *reinterpret_cast<const float2*>(posedirs + (size_t)r * (3 * V) + g);
        P[r * BT_COLS + cc] = x.x;
        P[r * BT_COLS + cc + 1] = x.y;
    }
    for (int i = t; i < BT_V * NJ; i += BT_THREADS)
        W[(i / NJ) * BT_WLD + i % NJ] = i < nv * NJ ? lbs_weights[(size_t)v0 * NJ + i] : 0.f;
    float sd[10], vt = 0.f;
#pragma unroll
    for (int l = 0; l < 10; ++l) sd[l] = gc < 3 * V ? shapedirs[(size_t)gc * 10 + l] : 0.f;
    if (gc < 3 * V) vt = v_template[gc];
    for (int n0 = 0; n0 < N; n0 += BT_ROWS) {
        __syncthreads();                                          // the pass before has read its rows
        for (int e = t; e < BT_ROWS * 207; e += BT_THREADS) {
            const int row = e / 207, r = e % 207;
            pfs[((row / BT_RB) * 207 + r) * BT_RB + row % BT_RB] =
                n0 + row < N ? work[(size_t)(n0 + row) * BW_ROW + BW_PF + r] : 0.f;
        }
        for (int e = t; e < BT_ROWS * NJ * 12; e += BT_THREADS) {
            const int row = e / (NJ * 12), i = e % (NJ * 12);
            As[e] = n0 + row < N ? work[(size_t)(n0 + row) * BW_ROW + BW_A + 16 * (i / 12) + i % 12] : 0.f;
        }
        for (int e = t; e < BT_ROWS * BT_PRM; e += BT_THREADS) {  // per row: betas [10], scale, transl [3]
            const int row = e / BT_PRM, q = e % BT_PRM;
            float x = 0.f;
            if (n0 + row < N && q < 14) x = params[(size_t)(n0 + row) * 86 + (q < 10 ? 76 + q : q - 10)];
            prm[e] = x;
        }
        __syncthreads();
        float acc[BT_RB] = {0.f, 0.f, 0.f, 0.f};
        const float4* pf4 = reinterpret_cast<const float4*>(pfs) + slot * 207;
        for (int q = 0; q < 207; ++q) {                           // lbs.py:201-202, the order of k_smpl_verts
            const float p = P[q * BT_COLS + c];
            const float4 f = pf4[q];
            acc[0] += f.x * p;
            acc[1] += f.y * p;
            acc[2] += f.z * p;
            acc[3] += f.w * p;
        }
#pragma unroll
        for (int k = 0; k < BT_RB; ++k) {
            const int row = slot * BT_RB + k;
            float a = 0.0f;
#pragma unroll
            for (int l = 0; l < 10; ++l) a += prm[row * BT_PRM + l] * sd[l];
            pv[row * BT_COLS + c] = acc[k] + (vt + a);
        }
        __syncthreads();
        for (int it = t; it < BT_ROWS * BT_V; it += BT_THREADS) {
            const int row = it / BT_V, vl = it % BT_V;
            if (n0 + row >= N || vl >= nv) continue;
            float T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = 0.f;
            for (int j = 0; j < NJ; ++j) {                        // lbs.py:217-221
                const float w = W[vl * BT_WLD + j];
#pragma unroll
                for (int i = 0; i < 12; ++i) T[i] += w * As[(row * NJ + j) * 12 + i];
            }
            const float* p = pv + row * BT_COLS + 3 * vl;
            const float scale = prm[row * BT_PRM + 10];
            float* out = verts + ((size_t)(n0 + row) * V + v0 + vl) * 3;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float x = T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3];
                out[a] = x * scale + prm[row * BT_PRM + 11 + a] * scale;  // smpl.py:77-78
            }
        }
    }
}
}  // namespace

extern "C" int mp_smpl_pose_batch(const float* v_template, const float* shapedirs, const float* posedirs,
                                  const float* j_regressor, const float* lbs_weights, const int* parents, const float* params,
                                  int N, const float* tfs_c_inv, float* verts, float* tfs, float* joints, float* work,
                                  void* stream) {
    if (N < 0 || !v_template || !shapedirs || !posedirs || !j_regressor || !lbs_weights || !parents) return -1;
    if (N == 0) return 0;
    if (!params || !work) return -1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smpl_batch_chain, dim3(N), dim3(256), 0, st, v_template, shapedirs, j_regressor, parents, params,
                       tfs_c_inv, work, tfs, joints);
    if (verts)
        hipLaunchKernelGGL(k_smpl_batch_verts, dim3(BT_BLOCKS), dim3(BT_THREADS), 0, st, posedirs, shapedirs, v_template,
                           lbs_weights, params, work, N, verts);
    return (int)hipGetLastError();
}

namespace {
// ---- adjoint of the posed vertices (mp_smpl_verts_bwd).  g_i = dverts_i, T_i = sum_j w_ij A_j, q_i = [p_i; 1]:
//   d scale = sum_i g_i . (T_i q_i + t) ; d transl = s sum_i g_i ; dA_j = s sum_i w_ij g_i (x) q_i ;
//   dp_i = s T_i[:3,:3]^T g_i -> dpf = posedirs dp, d betas = shapedirs^T dp.
// dp does not depend on p, so one pass over a tile of posedirs (207 rows x the 96 columns of 32 vertices, staged in LDS)
// gives both p (column sums) and the tile's share of dpf (row sums).  Each workgroup writes its 509 partial sums to its own
// scratch row; k_smpl_verts_bwd_finish adds the rows in a fixed order.
constexpr int VB = 32, VB_BLOCKS = (V + VB - 1) / VB, VB_COLS = 3 * VB, VB_LD = VB_COLS + 1, VB_ROW = 512;
constexpr int VB_PF = NJ * 12, VB_DS = VB_PF + 207, VB_DT = VB_DS + 1, VB_DB = VB_DT + 3, VB_OUT = VB_DB + 10;
static_assert(VB_BLOCKS * VB_ROW == MP_SMPL_VBWD_SCRATCH && VB_OUT <= VB_ROW && VB_COLS % 2 == 0 && (3 * V) % 2 == 0,
              "scratch layout of mp_smpl_verts_bwd");

__global__ __launch_bounds__(256) void k_smpl_verts_bwd(const float* __restrict__ posedirs,
                                                        const float* __restrict__ shapedirs,
                                                        const float* __restrict__ lbs_weights,
                                                        const float* __restrict__ params, const float* __restrict__ work,
                                                        const float* __restrict__ dverts, float* __restrict__ partial) {
    __shared__ float P[207 * VB_LD];
    __shared__ float A[NJ * 12], pf[207], W[VB * NJ], gs[VB_COLS], dp[VB_COLS], pv[VB_COLS], dsv[VB];
    const int t = threadIdx.x, v0 = blockIdx.x * VB, nv = min(VB, V - v0);
    float* out = partial + (size_t)blockIdx.x * VB_ROW;
    for (int i = t; i < NJ * 12; i += 256) A[i] = work[W_A + 16 * (i / 12) + i % 12];
    for (int i = t; i < 207; i += 256) pf[i] = work[W_PF + i];
    for (int i = t; i < VB * NJ; i += 256) W[i] = i < nv * NJ ? lbs_weights[(size_t)v0 * NJ + i] : 0.f;
    for (int e = t; e < 207 * (VB_COLS / 2); e += 256) {       // the tile, 8-byte loads (3V and the tile's first column are even)
        const int r = e / (VB_COLS / 2), c = 2 * (e % (VB_COLS / 2)), gc = 3 * v0 + c;
        float2 x = make_float2(0.f, 0.f);
        if (gc < 3 * V) x = *reinterpret_cast<const float2*>(posedirs + (size_t)r * (3 * V) + gc);
        P[r * VB_LD + c] = x.x;
        P[r * VB_LD + c + 1] = x.y;
    }
    __syncthreads();
    const float scale = params[0];
    float T[12], g[3] = {0.f, 0.f, 0.f};
    if (t < VB) {
        for (int i = 0; i < 12; ++i) T[i] = 0.f;
        for (int j = 0; j < NJ; ++j) {                          // the forward's blend, same order (k_smpl_verts)
            const float w = W[t * NJ + j];
            for (int i = 0; i < 12; ++i) T[i] += w * A[12 * j + i];
        }
        if (t < nv && dverts)
            for (int a = 0; a < 3; ++a) g[a] = dverts[3 * (size_t)(v0 + t) + a];
        for (int k = 0; k < 3; ++k) {
            dp[3 * t + k] = scale * (T[k] * g[0] + T[4 + k] * g[1] + T[8 + k] * g[2]);
            gs[3 * t + k] = scale * g[k];
        }
    }
    __syncthreads();
    if (t < VB_COLS) {                                          // p = v_shaped + posedirs^T pf  (lbs.py:201-202)
        float acc = 0.f;
        for (int r = 0; r < 207; ++r) acc += pf[r] * P[r * VB_LD + t];
        pv[t] = acc + (t < 3 * nv ? work[W_VS + 3 * v0 + t] : 0.f);
    } else if (t >= 128) {                                      // the tile's share of dpf = posedirs dp
        for (int r = t - 128; r < 207; r += 128) {
            float acc = 0.f;
            for (int c = 0; c < VB_COLS; ++c) acc += P[r * VB_LD + c] * dp[c];
            out[VB_PF + r] = acc;
        }
    }
    __syncthreads();
    if (t < VB) {
        float s = 0.f;
        for (int a = 0; a < 3; ++a)
            s += g[a] * (T[4 * a] * pv[3 * t] + T[4 * a + 1] * pv[3 * t + 1] + T[4 * a + 2] * pv[3 * t + 2] + T[4 * a + 3] +
                         params[1 + a]);
        dsv[t] = s;
    }
    __syncthreads();
    for (int e = t; e < NJ * 12 + 14; e += 256) {
        float acc = 0.f;
        if (e < NJ * 12) {                                      // dA_j[a][b] over the tile's vertices
            const int j = e / 12, a = (e % 12) / 4, b = e % 4;
            for (int i = 0; i < VB; ++i) acc += W[i * NJ + j] * gs[3 * i + a] * (b < 3 ? pv[3 * i + b] : 1.f);
            out[e] = acc;
        } else if (e == NJ * 12) {
            for (int i = 0; i < VB; ++i) acc += dsv[i];
            out[VB_DS] = acc;
        } else if (e < NJ * 12 + 4) {
            const int a = e - NJ * 12 - 1;
            for (int i = 0; i < VB; ++i) acc += gs[3 * i + a];
            out[VB_DT + a] = acc;
        } else {                                                // d betas through v_shaped (lbs.py:252-273)
            const int l = e - NJ * 12 - 4;
            for (int c = 0; c < 3 * nv; ++c) acc += shapedirs[(size_t)(3 * v0 + c) * 10 + l] * dp[c];
            out[VB_DB + l] = acc;
        }
    }
}

// sums the VB_BLOCKS partial rows (wave w: rows w, w + 4, ...; then the four waves in order) -> dlbs (MP_SMPL_DLBS layout)
__global__ __launch_bounds__(256) void k_smpl_verts_bwd_finish(const float* __restrict__ partial, float* __restrict__ dlbs) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, o = blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (o < VB_OUT)
        for (int r = wave; r < VB_BLOCKS; r += 4) acc += partial[(size_t)r * VB_ROW + o];
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0) return;
    const float s = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    if (o < NJ * 12) {
        const int j = o / 12, r = o % 12;
        dlbs[16 * j + r] = s;
        if (r < 4) dlbs[16 * j + 12 + r] = 0.f;
    } else if (o < VB_DS) dlbs[NJ * 16 + o - VB_PF] = s;
    else if (o < VB_DB) dlbs[NJ * 16 + 207 + o - VB_DS] = s;           // d scale, d transl
    else if (o < VB_OUT) dlbs[NJ * 16 + 207 + 76 + o - VB_DB] = s;     // d betas
    if (o < 72) dlbs[NJ * 16 + 207 + 4 + o] = 0.f;                       // thetas: through dA / dpf only
}
}  // namespace

extern "C" int mp_smpl_verts_bwd(const float* posedirs, const float* shapedirs, const float* lbs_weights, const float* params,
                                 const float* work, const float* dverts, float* scratch, float* dlbs, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_smpl_verts_bwd, dim3(VB_BLOCKS), dim3(256), 0, st, posedirs, shapedirs, lbs_weights, params, work,
                       dverts, scratch);
    hipLaunchKernelGGL(k_smpl_verts_bwd_finish, dim3((VB_OUT + 63) / 64), dim3(256), 0, st, scratch, dlbs);
    return (int)hipGetLastError();
}

namespace {
// ---- adjoint of SMPLServer.forward's bone transforms (smpl.py:50-94, lbs.py:276-377) w.r.t. the 86 SMPL parameters
//   [scale, transl(3), thetas(72), betas(10)];  one thread: 24 joints, a few hundred flops each.
//   Upstreams (each optional): dtfs (smpl_tfs), dA_ext (the rest-relative transforms A, from the posed vertices'
//   adjoint), djoints (smpl_jnts), dpf (the pose feature R_j - I, j >= 1), dparams_in (added at the end).
//   With only dtfs this is mp_smpl_pose_bwd: the hot path's samples reach the pose through the transforms alone.
__global__ void k_smpl_pose_bwd(const int* __restrict__ parents, const float* __restrict__ params,
                                const float* __restrict__ tfs_c_inv, const float* __restrict__ rest_joints,
                                const float* __restrict__ j_shapedirs, const float* __restrict__ dtfs,
                                const float* __restrict__ dA_ext, const float* __restrict__ djoints,
                                const float* __restrict__ dpf, const float* __restrict__ dparams_in,
                                float* __restrict__ dparams) {
    constexpr int NJ = 24;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float scale = params[0];
    const float* transl = params + 1;
    const float* th = params + 4;
    const float* J = rest_joints;
    float R[NJ][9], G[NJ][12], dG[NJ][12], dJ[NJ][3], dR[NJ][9];
    for (int j = 0; j < NJ; ++j) {
        const float ax = th[3 * j] + 1e-8f, ay = th[3 * j + 1] + 1e-8f, az = th[3 * j + 2] + 1e-8f;
        const float ang = sqrtf(ax * ax + ay * ay + az * az);
        const float n[3] = {th[3 * j] / ang, th[3 * j + 1] / ang, th[3 * j + 2] / ang};
        float s, c;
        sincosf(ang, &s, &c);
        const float K[9] = {0.f, -n[2], n[1], n[2], 0.f, -n[0], -n[1], n[0], 0.f};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                float kk = 0.f;
                for (int k = 0; k < 3; ++k) kk += K[3 * a + k] * K[3 * k + b];
                R[j][3 * a + b] = (a == b ? 1.f : 0.f) + s * K[3 * a + b] + (1.f - c) * kk;
            }
        const int p = parents[j];
        float rel[3];
        for (int a = 0; a < 3; ++a) rel[a] = J[3 * j + a] - (j > 0 ? J[3 * p + a] : 0.f);
        if (j == 0) {
            for (int a = 0; a < 3; ++a) { for (int b = 0; b < 3; ++b) G[0][4 * a + b] = R[0][3 * a + b]; G[0][4 * a + 3] = rel[a]; }
        } else {
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) {
                    float v = 0.f;
                    for (int k = 0; k < 3; ++k) v += G[p][4 * a + k] * R[j][3 * k + b];
                    G[j][4 * a + b] = v;
                }
                float v = G[p][4 * a + 3];
                for (int k = 0; k < 3; ++k) v += G[p][4 * a + k] * rel[k];
                G[j][4 * a + 3] = v;
            }
        }
        for (int a = 0; a < 3; ++a) dJ[j][a] = 0.f;
    }
    float dscale = 0.f, dtr[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < NJ; ++j) {
        // tfs_j = tf_j C_j  ->  d tf = dtfs C^T  (rows 0..2; C's last row is [0,0,0,1] for the absolute case C = I)
        float dtf[12];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) {
                float v = 0.f;
                if (dtfs && tfs_c_inv) for (int k = 0; k < 4; ++k) v += dtfs[16 * j + 4 * a + k] * tfs_c_inv[16 * j + 4 * b + k];
                else if (dtfs) v = dtfs[16 * j + 4 * a + b];
                dtf[4 * a + b] = v;
            }
        // A = G with translation column  A[a][3] = G[a][3] - sum_k G[a][k] J_j[k];  tf = scale A, tf[a][3] += scale transl[a]
        float dA[12];
        for (int a = 0; a < 3; ++a) {
            float A3 = G[j][4 * a + 3];
            for (int k = 0; k < 3; ++k) A3 -= G[j][4 * a + k] * J[3 * j + k];
            for (int b = 0; b < 3; ++b) dscale += dtf[4 * a + b] * G[j][4 * a + b];
            dscale += dtf[4 * a + 3] * (A3 + transl[a]);
            dtr[a] += scale * dtf[4 * a + 3];
            for (int b = 0; b < 4; ++b) dA[4 * a + b] = scale * dtf[4 * a + b];
            if (dA_ext)
                for (int b = 0; b < 4; ++b) dA[4 * a + b] += dA_ext[16 * j + 4 * a + b];
        }
        for (int a = 0; a < 3; ++a) {
            for (int k = 0; k < 3; ++k) {
                dG[j][4 * a + k] = dA[4 * a + k] - dA[4 * a + 3] * J[3 * j + k];
                dJ[j][k] -= dA[4 * a + 3] * G[j][4 * a + k];
            }
            dG[j][4 * a + 3] = dA[4 * a + 3];
        }
        if (djoints)      // joints_j = scale G_j[:3,3] + scale transl  (smpl.py:79-84)
            for (int a = 0; a < 3; ++a) {
                const float dj = djoints[3 * j + a];
                dscale += dj * (G[j][4 * a + 3] + transl[a]);
                dtr[a] += scale * dj;
                dG[j][4 * a + 3] += scale * dj;
            }
    }
    // The recursion is smpl_chain.hpp's, shared with the keypoint fit (keypoint_fit.hip).  Rodrigues, the forward chain, the seed
    // above and Rodrigues' adjoint below stay written out here although the header has them too: routed through the header's
    // functions the compiler contracted their multiply-adds differently (other fma / mul / add counts in the kernel), and
    // mp_smpl_pose_bwd* keeps its bits.
    for (int j = NJ - 1; j >= 1; --j)     // G_j = G_p [R_j | rel_j]
        mp::smpl_chain_joint_adjoint(j, parents[j], J, R, G, dG, dJ, dR);
    mp::smpl_chain_root_adjoint(dG, dJ, dR);
    if (dpf)              // pose_feature = (R_j - I).flatten, j >= 1 (lbs.py:199)
        for (int j = 1; j < NJ; ++j)
            for (int e = 0; e < 9; ++e) dR[j][e] += dpf[9 * (j - 1) + e];
    for (int i = 0; i < 86; ++i) dparams[i] = 0.f;
    dparams[0] = dscale;
    for (int a = 0; a < 3; ++a) dparams[1 + a] = dtr[a];
    for (int j = 0; j < NJ; ++j) {   // Rodrigues with angle = |theta + 1e-8|, axis = theta / angle (lbs.py:290-296)
        const float t3[3] = {th[3 * j], th[3 * j + 1], th[3 * j + 2]};
        const float e3[3] = {t3[0] + 1e-8f, t3[1] + 1e-8f, t3[2] + 1e-8f};
        const float ang = sqrtf(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
        const float n[3] = {t3[0] / ang, t3[1] / ang, t3[2] / ang};
        float s, c;
        sincosf(ang, &s, &c);
        const float K[9] = {0.f, -n[2], n[1], n[2], 0.f, -n[0], -n[1], n[0], 0.f};
        float KK[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                float kk = 0.f;
                for (int k = 0; k < 3; ++k) kk += K[3 * a + k] * K[3 * k + b];
                KK[3 * a + b] = kk;
            }
        float dang = 0.f;
        for (int e = 0; e < 9; ++e) dang += dR[j][e] * (c * K[e] + s * KK[e]);
        // dK (adjoint of K): from s K and (1-c) K K  ->  dK = s dR + (1-c) (dR K^T + K^T dR)
        float dK[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                float v = s * dR[j][3 * a + b];
                for (int k = 0; k < 3; ++k) v += (1.f - c) * (dR[j][3 * a + k] * K[3 * b + k] + K[3 * k + a] * dR[j][3 * k + b]);
                dK[3 * a + b] = v;
            }
        const float dn[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
        float ndot = 0.f;
        for (int k = 0; k < 3; ++k) ndot += dn[k] * t3[k];
        for (int i = 0; i < 3; ++i)
            dparams[4 + 3 * j + i] = dang * e3[i] / ang + dn[i] / ang - ndot * e3[i] / (ang * ang * ang);
    }
    if (j_shapedirs)
        for (int l = 0; l < 10; ++l) {
            float v = 0.f;
            for (int j = 0; j < NJ; ++j)
                for (int k = 0; k < 3; ++k) v += dJ[j][k] * j_shapedirs[(3 * j + k) * 10 + l];
            dparams[76 + l] = v;
        }
    if (dparams_in)
        for (int i = 0; i < 86; ++i) dparams[i] += dparams_in[i];
}
}  // namespace

extern "C" int mp_smpl_pose_bwd(const int* parents, const float* params, const float* tfs_c_inv, const float* rest_joints,
                                const float* j_shapedirs, const float* dtfs, float* dparams, void* stream) {
    hipLaunchKernelGGL(k_smpl_pose_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, parents, params, tfs_c_inv, rest_joints, j_shapedirs, dtfs,
                       nullptr, nullptr, nullptr, nullptr, dparams);
    return (int)hipGetLastError();
}

extern "C" int mp_smpl_pose_bwd_lbs(const int* parents, const float* params, const float* tfs_c_inv, const float* rest_joints,
                                    const float* j_shapedirs, const float* dtfs, const float* dA, const float* djoints,
                                    const float* dpf, const float* dparams_in, float* dparams, void* stream) {
    hipLaunchKernelGGL(k_smpl_pose_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, parents, params, tfs_c_inv, rest_joints, j_shapedirs, dtfs,
                       dA, djoints, dpf, dparams_in, dparams);
    return (int)hipGetLastError();
}
