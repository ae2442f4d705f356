// Refining SMPL fits to 2D keypoints (mp_kp_objective, mp_kp_fit): the objective of the reference's `refine` mode
// (preprocessing/preprocessing_multiple_trace.py:360-527, preprocessing/loss.py) with its adjoint and the Adam loop, one workgroup
// per person-frame, all steps in one launch.  Entry points and layouts: include/multiply_hip.h.
//
// One evaluation (kp_eval, all 256 threads of the workgroup; every phase ends at a barrier):
//   0  rest joints J (72 threads), Rodrigues (24 lanes, mp::smpl_rodrigues)
//   1  the chain on lane 0 (mp::smpl_chain_joint), the pose feature on the other waves
//   2  rest-relative transforms A and posed joints (24 lanes); posedirs^T pf for the support vertices: wave w sums the terms
//      [52 w, 52 w + 52) of its columns (lanes over the columns: coalesced), the four partial sums are added in wave order
//   3  v_posed = (v_template + shapedirs betas) + the four partials
//   4  skinning, one thread per support vertex
//   5  wave 0: keypoints (one lane each: map, projection, robust residual, its adjoint) and their sum; wave 1: the temporal term
//   6  adjoint of the map: one thread per source gathers its keypoints (the transposed map)
//   7  adjoint of the skinning: d v_posed per vertex
//   8  dA (one thread per entry, vertices in order), d pose feature (wave per row range, lanes over the columns, wave sum),
//      d betas through the vertices, d transl
//   9  the chain adjoint on lane 0 (mp::smpl_rel_transform_adjoint, mp::smpl_chain_joint_adjoint: the arithmetic of
//      k_smpl_pose_bwd, csrc/smpl_chain.hpp)
//   10 Rodrigues' adjoint (24 lanes), d betas through the rest joints, the gradient row
// Every sum has a fixed order that depends on S and K alone: no atomics, the same bits on every call and at every place in a batch.
#include <hip/hip_runtime.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "smpl_chain.hpp"

namespace {
constexpr int NJ = MP_SMPL_J, NP = MP_KP_PARAMS, MAXK = MP_KP_MAX_K, MAXS = MP_KP_MAX_S, NT = 256, PFQ = 52;
constexpr int P_TR = 0, P_TH = 3, P_BE = 75;
static_assert(MAXK <= 64 && 4 * PFQ >= 207 && NP == 85, "one wave holds the keypoints; four waves split the pose feature");

struct KpTables {
    const int* parents;
    const float *j_template, *j_shapedirs, *sv_template, *s_shapedirs, *s_posedirs, *s_weights;   // of the row's table set
    const int *map_ptr, *map_idx, *tmap_ptr, *tmap_k;
    const float *map_w, *tmap_w;
    int S, K;
};
struct KpRow {
    const float *targets, *c, *cam;   // [K][2], [K], [16]
    bool temporal;
    float rho, w_2d, w_t, w_p;
};
struct KpShared {
    float prm[NP], grad[NP];
    float J[3 * NJ], R[NJ][9], G[NJ][12], A[NJ][12], pf[207];
    float Rprev[NJ][9], tprev[3];
    float dG[NJ][12], dR[NJ][9], dJ[NJ][3], dA[NJ][12], dpf[207], dRt[NJ][6], dtr[3], dbv[10];
    float p[3 * MAXS], dp[3 * MAXS], part[4][3 * MAXS];
    float src[3 * (NJ + MAXS)], dsrc[3 * (NJ + MAXS)];
    float dX[3 * MAXK], proj[2 * MAXK];
    float terms[3], l2d, lp, lt;
    int flag;
};
static_assert(sizeof(KpShared) <= 40 * 1024, "the row's state: 38 KB of LDS");

// T = sum_j w_j A_j of support vertex s (lbs.py:217-221, the order of k_smpl_verts)
__device__ __forceinline__ void kp_blend(const KpTables& tb, const KpShared& sh, int s, float* T) {
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.f;
    for (int j = 0; j < NJ; ++j) {
        const float w = tb.s_weights[(size_t)s * NJ + j];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] += w * sh.A[j][i];
    }
}

// the objective of the parameters in sh.prm: sh.terms, sh.proj, sh.flag (or-ed), and with want_grad sh.grad.  All threads call.
__device__ __forceinline__ void kp_eval(const KpTables& tb, const KpRow& row, KpShared& sh, bool want_grad) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int S = tb.S, K = tb.K, S3 = 3 * S;
    const float* betas = sh.prm + P_BE;
    // ---- 0
    if (t < 3 * NJ) {
        float a = 0.f;
#pragma unroll
        for (int l = 0; l < 10; ++l) a += betas[l] * tb.j_shapedirs[t * 10 + l];
        sh.J[t] = tb.j_template[t] + a;
    }
    if (t < NJ) mp::smpl_rodrigues(sh.prm + P_TH + 3 * t, sh.R[t]);
    __syncthreads();
    // ---- 1
    if (t == 0)
        for (int j = 0; j < NJ; ++j) mp::smpl_chain_joint(j, tb.parents[j], sh.J, sh.R, sh.G);
    if (t >= 64)
        for (int i = t - 64; i < 207; i += NT - 64) {   // pose_feature = (R[1:] - I).flatten (lbs.py:199)
            const int e = i % 9;
            sh.pf[i] = sh.R[i / 9 + 1][e] - ((e % 4 == 0) ? 1.0f : 0.0f);
        }
    __syncthreads();
    // ---- 2
    if (t < NJ) {
        for (int a = 0; a < 3; ++a) {
            float s = 0.f;
            for (int k = 0; k < 3; ++k) {
                sh.A[t][4 * a + k] = sh.G[t][4 * a + k];
                s += sh.G[t][4 * a + k] * sh.J[3 * t + k];
            }
            sh.A[t][4 * a + 3] = sh.G[t][4 * a + 3] - s;   // rel_transforms = G - pad(G @ [J;0])  (lbs.py:372-375)
            sh.src[3 * t + a] = sh.G[t][4 * a + 3] + sh.prm[P_TR + a];
        }
    }
    {
        const int q0 = wave * PFQ, q1 = min(207, q0 + PFQ);
        for (int e = lane; e < S3; e += 64) {
            float acc = 0.f;
            for (int q = q0; q < q1; ++q) acc += sh.pf[q] * tb.s_posedirs[(size_t)q * S3 + e];   // lbs.py:201-202
            sh.part[wave][e] = acc;
        }
    }
    __syncthreads();
    // ---- 3
    for (int e = t; e < S3; e += NT) {
        float a = 0.f;
#pragma unroll
        for (int l = 0; l < 10; ++l) a += betas[l] * tb.s_shapedirs[(size_t)e * 10 + l];   // blend_shapes, lbs.py:252-273
        sh.p[e] = (tb.sv_template[e] + a) + (((sh.part[0][e] + sh.part[1][e]) + sh.part[2][e]) + sh.part[3][e]);
    }
    __syncthreads();
    // ---- 4
    for (int s = t; s < S; s += NT) {
        float T[12];
        kp_blend(tb, sh, s, T);
        const float* p = sh.p + 3 * s;
        for (int a = 0; a < 3; ++a)
            sh.src[3 * (NJ + s) + a] = (T[4 * a] * p[0] + T[4 * a + 1] * p[1] + T[4 * a + 2] * p[2] + T[4 * a + 3]) + sh.prm[P_TR + a];
    }
    __syncthreads();
    // ---- 5
    if (wave == 0) {
        float lk = 0.f;
        if (lane < K) {
            float X[3] = {0.f, 0.f, 0.f};
            for (int m = tb.map_ptr[lane]; m < tb.map_ptr[lane + 1]; ++m) {
                const int i = tb.map_idx[m];
                if ((unsigned)i >= (unsigned)(NJ + S)) continue;
                const float a = tb.map_w[m];
                for (int d = 0; d < 3; ++d) X[d] += a * sh.src[3 * i + d];
            }
            const float* cam = row.cam;
            float xc[3];
            for (int a = 0; a < 3; ++a) xc[a] = cam[4 + 4 * a] * X[0] + cam[5 + 4 * a] * X[1] + cam[6 + 4 * a] * X[2] + cam[7 + 4 * a];
            float dxc[3] = {0.f, 0.f, 0.f}, u = 0.f, v = 0.f;
            if (xc[2] > 0.f) {
                const float iz = 1.0f / xc[2], fx = cam[0], fy = cam[1], ck = row.c[lane], r2 = row.rho * row.rho;
                u = fx * xc[0] * iz + cam[2];
                v = fy * xc[1] * iz + cam[3];
                const float ru = row.targets[2 * lane] - u, rv = row.targets[2 * lane + 1] - v;
                const float du_ = ru * ru + r2, dv_ = rv * rv + r2;
                lk = ck * (r2 * (ru * ru) / du_ + r2 * (rv * rv) / dv_);        // GMoF (preprocessing_utils.py:218-229)
                // d lk / d u = -c rho^4 2 r / (r^2 + rho^2)^2, times w_2d
                const float gu = -row.w_2d * ck * 2.0f * ru * (r2 / du_) * (r2 / du_);
                const float gv = -row.w_2d * ck * 2.0f * rv * (r2 / dv_) * (r2 / dv_);
                dxc[0] = gu * fx * iz;
                dxc[1] = gv * fy * iz;
                dxc[2] = -(gu * fx * xc[0] + gv * fy * xc[1]) * iz * iz;
            } else {
                sh.flag = 1;      // (every writer writes 1)
            }
            sh.proj[2 * lane] = u;
            sh.proj[2 * lane + 1] = v;
            for (int b = 0; b < 3; ++b) sh.dX[3 * lane + b] = cam[4 + b] * dxc[0] + cam[8 + b] * dxc[1] + cam[12 + b] * dxc[2];
        }
        lk = mp::wsum(lk);
        if (lane == 0) sh.l2d = lk;
    } else if (wave == 1) {
        float lp = 0.f, lt = 0.f;
        if (row.temporal) {
            if (lane < NJ) {
                for (int a = 0; a < 3; ++a)
                    for (int b = 0; b < 2; ++b) {
                        const float d = sh.R[lane][3 * a + b] - sh.Rprev[lane][3 * a + b];
                        lp += d * d;
                        sh.dRt[lane][2 * a + b] = row.w_t * row.w_p * (2.0f / 144.0f) * d;
                    }
            } else if (lane < NJ + 3) {
                const float d = sh.prm[P_TR + lane - NJ] - sh.tprev[lane - NJ];
                lt = d * d;
                sh.dtr[lane - NJ] = row.w_t * (2.0f / 3.0f) * d;
            }
        } else if (lane < NJ) {
            for (int e = 0; e < 6; ++e) sh.dRt[lane][e] = 0.f;
        } else if (lane < NJ + 3) {
            sh.dtr[lane - NJ] = 0.f;
        }
        lp = mp::wsum(lp);
        lt = mp::wsum(lt);
        if (lane == 0) { sh.lp = lp * (1.0f / 144.0f); sh.lt = lt * (1.0f / 3.0f); }
    }
    __syncthreads();
    if (t == 0) {
        const float ltemp = row.w_p * sh.lp + sh.lt;
        sh.terms[0] = sh.l2d;
        sh.terms[1] = ltemp;
        sh.terms[2] = row.w_2d * sh.l2d + row.w_t * ltemp;
    }
    if (!want_grad) { __syncthreads(); return; }
    // ---- 6
    for (int i = t; i < NJ + S; i += NT) {
        float g[3] = {0.f, 0.f, 0.f};
        for (int m = tb.tmap_ptr[i]; m < tb.tmap_ptr[i + 1]; ++m) {
            const int k = tb.tmap_k[m];
            if ((unsigned)k >= (unsigned)K) continue;
            const float a = tb.tmap_w[m];
            for (int d = 0; d < 3; ++d) g[d] += a * sh.dX[3 * k + d];
        }
        for (int d = 0; d < 3; ++d) sh.dsrc[3 * i + d] = g[d];
    }
    __syncthreads();
    // ---- 7
    for (int s = t; s < S; s += NT) {
        float T[12];
        kp_blend(tb, sh, s, T);
        const float* g = sh.dsrc + 3 * (NJ + s);
        for (int k = 0; k < 3; ++k) sh.dp[3 * s + k] = T[k] * g[0] + T[4 + k] * g[1] + T[8 + k] * g[2];
    }
    __syncthreads();
    // ---- 8
    for (int e = t; e < NJ * 12; e += NT) {   // dA_j[a][b] = sum_s w_sj g_s[a] [p_s; 1][b]
        const int j = e / 12, a = (e % 12) / 4, b = e % 4;
        float acc = 0.f;
        for (int s = 0; s < S; ++s)
            acc += tb.s_weights[(size_t)s * NJ + j] * sh.dsrc[3 * (NJ + s) + a] * (b < 3 ? sh.p[3 * s + b] : 1.f);
        sh.dA[j][4 * a + b] = acc;
    }
    {
        const int q0 = wave * PFQ, q1 = min(207, q0 + PFQ);
        for (int q = q0; q < q1; ++q) {       // d pf = posedirs dp
            float acc = 0.f;
            for (int e = lane; e < S3; e += 64) acc += tb.s_posedirs[(size_t)q * S3 + e] * sh.dp[e];
            acc = mp::wsum(acc);
            if (lane == 0) sh.dpf[q] = acc;
        }
        for (int l = wave; l < 10; l += 4) {  // d betas through v_shaped (lbs.py:252-273)
            float acc = 0.f;
            for (int e = lane; e < S3; e += 64) acc += tb.s_shapedirs[(size_t)e * 10 + l] * sh.dp[e];
            acc = mp::wsum(acc);
            if (lane == 0) sh.dbv[l] = acc;
        }
    }
    if (t >= NT - 3) {                         // d transl: every source moves with it
        const int a = t - (NT - 3);
        float acc = sh.dtr[a];
        for (int i = 0; i < NJ + S; ++i) acc += sh.dsrc[3 * i + a];
        sh.grad[P_TR + a] = acc;
    }
    __syncthreads();
    // ---- 9
    if (t == 0) {
        for (int j = 0; j < NJ; ++j)
            for (int a = 0; a < 3; ++a) sh.dJ[j][a] = 0.f;
        for (int j = 0; j < NJ; ++j) {
            mp::smpl_rel_transform_adjoint(j, sh.dA[j], sh.J, sh.G, sh.dG, sh.dJ);
            for (int a = 0; a < 3; ++a) sh.dG[j][4 * a + 3] += sh.dsrc[3 * j + a];   // posed joint j = G_j[:3,3] + transl
        }
        for (int j = NJ - 1; j >= 1; --j) mp::smpl_chain_joint_adjoint(j, tb.parents[j], sh.J, sh.R, sh.G, sh.dG, sh.dJ, sh.dR);
        mp::smpl_chain_root_adjoint(sh.dG, sh.dJ, sh.dR);
    }
    __syncthreads();
    // ---- 10
    if (t < NJ) {
        float dR[9];
        for (int e = 0; e < 9; ++e) dR[e] = sh.dR[t][e] + (t > 0 ? sh.dpf[9 * (t - 1) + e] : 0.f);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 2; ++b) dR[3 * a + b] += sh.dRt[t][2 * a + b];
        mp::smpl_rodrigues_adjoint(sh.prm + P_TH + 3 * t, dR, sh.grad + P_TH + 3 * t);
    } else if (t >= 64 && t < 74) {
        const int l = t - 64;
        float acc = sh.dbv[l];
        for (int e = 0; e < 3 * NJ; ++e) acc += sh.dJ[e / 3][e % 3] * tb.j_shapedirs[e * 10 + l];
        sh.grad[P_BE + l] = acc;
    }
    __syncthreads();
}

struct KpArgs {
    KpTables tb;            // table pointers of set 0
    int n_tables;
    const int* row_table;
    const float *params, *prev, *targets, *c, *camera;
    float rho, w_2d, w_t, w_p;
};

// the row's tables, inputs and start values -> tb, row, sh (all threads; ends at a barrier)
__device__ __forceinline__ void kp_load(const KpArgs& a, size_t n, KpTables& tb, KpRow& row, KpShared& sh) {
    const int t = threadIdx.x;
    tb = a.tb;
    int ts = a.row_table ? a.row_table[n] : 0;
    if (ts < 0 || ts >= a.n_tables) ts = 0;
    const size_t S = tb.S;
    tb.j_template += (size_t)ts * 3 * NJ;
    tb.j_shapedirs += (size_t)ts * 3 * NJ * 10;
    tb.sv_template += ts * S * 3;
    tb.s_shapedirs += ts * S * 30;
    tb.s_posedirs += ts * S * 3 * 207;
    tb.s_weights += ts * S * NJ;
    row.targets = a.targets + n * tb.K * 2;
    row.c = a.c + n * tb.K;
    row.cam = a.camera + n * 16;
    row.temporal = a.prev != nullptr;
    row.rho = a.rho; row.w_2d = a.w_2d; row.w_t = a.w_t; row.w_p = a.w_p;
    if (t < NP) sh.prm[t] = a.params[n * NP + t];
    if (t == NT - 1) sh.flag = 0;
    if (a.prev && t >= 64 && t < 64 + NJ) mp::smpl_rodrigues(a.prev + n * 75 + 3 + 3 * (t - 64), sh.Rprev[t - 64]);
    if (a.prev && t >= 128 && t < 131) sh.tprev[t - 128] = a.prev[n * 75 + t - 128];
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_kp_objective(KpArgs a, float* __restrict__ terms, float* __restrict__ grad,
                                                     float* __restrict__ proj, int* __restrict__ flags) {
    __shared__ KpShared sh;
    KpTables tb;
    KpRow row;
    const size_t n = blockIdx.x;
    const int t = threadIdx.x;
    kp_load(a, n, tb, row, sh);
    kp_eval(tb, row, sh, grad != nullptr);
    if (terms && t < 3) terms[n * 3 + t] = sh.terms[t];
    if (grad && t < NP) grad[n * NP + t] = sh.grad[t];
    if (proj && t < 2 * tb.K) proj[n * 2 * tb.K + t] = sh.proj[t];
    if (t == 0) flags[n] = sh.flag;
}

__global__ __launch_bounds__(NT) void k_kp_fit(KpArgs a, int iters, float lr_t, float lr_p, float lr_b, float beta1, float beta2,
                                               float eps, float* __restrict__ out, float* __restrict__ history,
                                               int* __restrict__ flags) {
    __shared__ KpShared sh;
    KpTables tb;
    KpRow row;
    const size_t n = blockIdx.x;
    const int t = threadIdx.x;
    kp_load(a, n, tb, row, sh);
    // torch.optim.Adam (single tensor form): thread i owns parameter i and its two moments; the bias corrections are doubles
    // as the python scalars of torch's step are
    float m = 0.f, v = 0.f;
    const float lr = t < P_TH ? lr_t : (t < P_BE ? lr_p : lr_b);
    double b1t = 1.0, b2t = 1.0;
    for (int it = 0; it < iters; ++it) {
        kp_eval(tb, row, sh, true);
        if (history && t < 3) history[(n * iters + it) * 3 + t] = sh.terms[t];
        b1t *= (double)beta1;
        b2t *= (double)beta2;
        if (t < NP) {
            const float g = sh.grad[t];
            // (explicit fused multiply-adds: the rounding of a step is spelled out, not left to the compiler's contraction)
            m = fmaf(g - m, 1.0f - beta1, m);                       // exp_avg.lerp_(grad, 1 - beta1)
            v = fmaf(v, beta2, ((1.0f - beta2) * g) * g);           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
            const float step = (float)((double)lr / (1.0 - b1t));
            const float bc2 = (float)sqrt(1.0 - b2t);
            const float denom = sqrtf(v) / bc2 + eps;
            sh.prm[t] = fmaf(-step, m / denom, sh.prm[t]);          // param.addcdiv_(exp_avg, denom, value=-step_size)
        }
        __syncthreads();
    }
    if (t < NP) out[n * NP + t] = sh.prm[t];
    if (t == 0) flags[n] = sh.flag;
}

int kp_args(KpArgs& a, const int* parents, const float* j_template, const float* j_shapedirs, const float* sv_template,
            const float* s_shapedirs, const float* s_posedirs, const float* s_weights, int n_tables, const int* row_table,
            const int* map_ptr, const int* map_idx, const float* map_w, const int* tmap_ptr, const int* tmap_k,
            const float* tmap_w, int S, int K, const float* params, const float* prev, const float* targets, const float* c,
            const float* camera, int N, float rho, float w_2d, float w_t, float w_p, const int* flags) {
    if (N < 0 || n_tables < 1) return -1;
    if (K < 1 || K > MAXK || S < 0 || S > MAXS) return -2;
    if (!parents || !j_template || !j_shapedirs || !map_ptr || !map_idx || !map_w || !tmap_ptr || !tmap_k || !tmap_w) return -1;
    if (S > 0 && (!sv_template || !s_shapedirs || !s_posedirs || !s_weights)) return -1;
    if (N > 0 && (!params || !targets || !c || !camera || !flags)) return -1;
    a.tb = KpTables{parents, j_template, j_shapedirs, sv_template, s_shapedirs, s_posedirs, s_weights,
                    map_ptr, map_idx, tmap_ptr, tmap_k, map_w, tmap_w, S, K};
    a.n_tables = n_tables;
    a.row_table = row_table;
    a.params = params; a.prev = prev; a.targets = targets; a.c = c; a.camera = camera;
    a.rho = rho; a.w_2d = w_2d; a.w_t = w_t; a.w_p = w_p;
    return 0;
}
}  // namespace

extern "C" int mp_kp_objective(const int* parents, const float* j_template, const float* j_shapedirs, const float* sv_template,
                               const float* s_shapedirs, const float* s_posedirs, const float* s_weights, int n_tables,
                               const int* row_table, const int* map_ptr, const int* map_idx, const float* map_w,
                               const int* tmap_ptr, const int* tmap_k, const float* tmap_w, int S, int K, const float* params,
                               const float* prev, const float* targets, const float* c, const float* camera, int N, float rho,
                               float w_2d, float w_t, float w_p, float* terms, float* grad, float* proj, int* flags,
                               void* stream) {
    KpArgs a;
    const int rc = kp_args(a, parents, j_template, j_shapedirs, sv_template, s_shapedirs, s_posedirs, s_weights, n_tables, row_table,
                           map_ptr, map_idx, map_w, tmap_ptr, tmap_k, tmap_w, S, K, params, prev, targets, c, camera, N, rho, w_2d,
                           w_t, w_p, flags);
    if (rc || N == 0) return rc;
    hipLaunchKernelGGL(k_kp_objective, dim3(N), dim3(NT), 0, (hipStream_t)stream, a, terms, grad, proj, flags);
    return (int)hipGetLastError();
}

extern "C" int mp_kp_fit(const int* parents, const float* j_template, const float* j_shapedirs, const float* sv_template,
                         const float* s_shapedirs, const float* s_posedirs, const float* s_weights, int n_tables,
                         const int* row_table, const int* map_ptr, const int* map_idx, const float* map_w, const int* tmap_ptr,
                         const int* tmap_k, const float* tmap_w, int S, int K, const float* params, const float* prev,
                         const float* targets, const float* c, const float* camera, int N, float rho, float w_2d, float w_t,
                         float w_p, int iters, float lr_t, float lr_p, float lr_b, float beta1, float beta2, float eps,
                         float* out, float* history, int* flags, void* stream) {
    KpArgs a;
    const int rc = kp_args(a, parents, j_template, j_shapedirs, sv_template, s_shapedirs, s_posedirs, s_weights, n_tables, row_table,
                           map_ptr, map_idx, map_w, tmap_ptr, tmap_k, tmap_w, S, K, params, prev, targets, c, camera, N, rho, w_2d,
                           w_t, w_p, flags);
    if (rc) return rc;
    if (iters < 0 || (N > 0 && !out)) return -1;
    if (N == 0) return 0;
    hipLaunchKernelGGL(k_kp_fit, dim3(N), dim3(NT), 0, (hipStream_t)stream, a, iters, lr_t, lr_p, lr_b, beta1, beta2, eps, out,
                       history, flags);
    return (int)hipGetLastError();
}
