// Multi-person compositing (reference code/lib/model/multiply.py:425-480, 544-545, 590), its geometry outputs and their adjoints.
// The reference packs every person's samples into one list, radix-sorts it twice (by t_end, then stably by ray) and
// calls nerfacc's packed scan; the arithmetic per sample is nerfacc's render_weight_from_density: with fe = sigma dt the free
// energy of a sample and E the sum of fe over the samples in front of it in the merged order,
//   alpha = 1 - exp(-fe),  T = exp(-E),  w = alpha T.
// Here ONE WAVE owns one ray and nothing is merged: mp::RayMerge (ray_merge.hpp) holds the per-person LDS arrays, their fill
// (phase 1), the rank search with its tie rule, the free energy in front of a sample and the last-sample rule.  Rows are read
// with coalesced 64-lane loads (the first version, one thread per ray walking its rows, moved 15x the algorithmic bytes through
// HBM: profiles/r01_pmc_traffic.txt), prefix sums are wave scans.  The four kernels and what each adds to that core:
//   k_composite               sums w rgb, w normal, w (merged and per person); T_bg from the last-sample rule.  No LDS extras:
//                             3S+1 floats per person.
//   k_composite_geometry      sums w t_mid (merged and per person), the person's own ("solo") opacity and depth, and the depth at
//                             which the free energy reaches a level, merged and solo.  No LDS extras: 3S+1.
//   k_composite_bwd           adjoint of k_composite into sdf, rgb, bg_rgb and beta.  Extras: gp [S+1], the prefix sums of dw w,
//                             and w [S]: 5S+2.
//   k_composite_geometry_bwd  adjoint of k_composite_geometry's differentiable outputs into sdf and beta.  Extras: gm [S+1], the
//                             prefix sums of dw w in the merged order, and gs [S+1], those of dws w0 in the person's own: 5S+3.
// The forward kernels run 4 waves per block; the adjoints halve that until their larger LDS fits (launch_shape).
#include <hip/hip_runtime.h>
#include <float.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "ray_merge.hpp"

namespace {

using mp::MAX_P;
using mp::RayMerge;

constexpr int WPB = 4;   // rays (waves) per workgroup, at most
constexpr int LDS_MAX = 160 * 1024;

// floats per person in LDS, per kernel
constexpr int fwd_stride(int S) { return RayMerge::prefix_floats(S); }
constexpr int bwd_stride(int S) { return RayMerge::prefix_floats(S) + (S + 1) + S; }
constexpr int geometry_bwd_stride(int S) { return RayMerge::prefix_floats(S) + 2 * (S + 1); }

__global__ __launch_bounds__(64 * WPB) void k_composite(int n_rays, int P, int n_z, const int* const* __restrict__ inv_index,
                                                       const float* const* __restrict__ z,
                                                       const float* const* __restrict__ sdf,
                                                       const float* const* __restrict__ rgb,
                                                       const float* const* __restrict__ normal,
                                                       const float* __restrict__ beta_p, const float* __restrict__ bg_rgb,
                                                       float* __restrict__ rgb_values, float* __restrict__ fg_rgb_values,
                                                       float* __restrict__ normal_values, float* __restrict__ acc_map,
                                                       float* __restrict__ acc_person, float* __restrict__ bg_T) {
    extern __shared__ float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WPB + wave;
    const int S = n_z - 1;
    const bool live = r < n_rays;
    const RayMerge m(smem, wave, S, fwd_stride(S), P, live, r, inv_index);
    m.fill(z, sdf, *beta_p);

    // ---- phase 2: weights and accumulation
    float c[3] = {0.f, 0.f, 0.f}, nn[3] = {0.f, 0.f, 0.f}, acc = 0.f, accp[MAX_P];
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) accp[p] = 0.f;
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        if (m.has(p)) {
            const float* fe_l = m.fe(p);
            for (int i = lane; i < S; i += 64) {
                const float fe = fe_l[i];
                const float T = expf(-m.energy_in_front(p, i));
                const float w = (1.0f - expf(-fe)) * T;
                if (w != 0.0f) {  // skipped samples carry undefined colour/normal but exactly zero weight
                    const size_t qi = (size_t)m.k[p] * S + i;
                    c[0] += w * rgb[p][3 * qi]; c[1] += w * rgb[p][3 * qi + 1]; c[2] += w * rgb[p][3 * qi + 2];
                    nn[0] += w * normal[p][3 * qi]; nn[1] += w * normal[p][3 * qi + 1]; nn[2] += w * normal[p][3 * qi + 2];
                }
                acc += w;
                accp[p] += w;
            }
        }
    }
    for (int a = 0; a < 3; ++a) { c[a] = mp::wsum(c[a]); nn[a] = mp::wsum(nn[a]); }
    acc = mp::wsum(acc);
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) accp[p] = mp::wsum(accp[p]);
    if (!live || lane != 0) return;
    float T_last;
    m.last_sample(T_last);
    bg_T[r] = T_last;
    acc_map[r] = acc;
    for (int p = 0; p < P; ++p) acc_person[(size_t)r * P + p] = accp[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float bg = bg_rgb ? bg_rgb[3 * r + a] : 1.0f;     // multiply.py:541
        rgb_values[3 * r + a] = c[a] + T_last * bg;             // :544-545
        fg_rgb_values[3 * r + a] = c[a] + T_last * 1.0f;        // :590
        normal_values[3 * r + a] = nn[a];
    }
}

// Geometry of the same merge: where along the ray the volume is, instead of what colour it has.  Phase 2 sums w * t_mid (merged
// and per person), the person's own ("solo": as if rendered alone, E = its own prefix sum) opacity and depth, and finds the
// depth at which the free energy reaches L = -ln(1 - level): the FIRST sample in merged order with E + fe >= L, found as the
// minimum of the key (t_end, person, sample) over every sample that satisfies the inequality (in fp32 the per-person sums of E
// do not tile the axis, the minimum is defined regardless), linearly interpolated inside that sample.  Every lane keeps its best
// candidate; the wave reduces on t_end, then on the person among the lanes holding the minimum, then on the sample index.
// No atomics, fixed summation order: bit-identical from run to run.  Any output pointer may be null.
__device__ __forceinline__ float level_depth(float ts, float te, float E, float fe, float L) {
    const float f = fe > 0.f ? fminf(fmaxf((L - E) / fe, 0.f), 1.f) : 0.f;
    return ts + (te - ts) * f;
}

__global__ __launch_bounds__(64 * WPB) void k_composite_geometry(int n_rays, int P, int n_z, const int* const* __restrict__ inv_index,
                                                                const float* const* __restrict__ z,
                                                                const float* const* __restrict__ sdf,
                                                                const float* __restrict__ beta_p, float L,
                                                                float* __restrict__ depth, float* __restrict__ depth_person,
                                                                float* __restrict__ depth_level, int* __restrict__ front_person,
                                                                float* __restrict__ acc_solo, float* __restrict__ depth_solo,
                                                                float* __restrict__ depth_solo_level) {
    extern __shared__ float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * WPB + wave;
    const int S = n_z - 1;
    const bool live = r < n_rays;
    const RayMerge m(smem, wave, S, fwd_stride(S), P, live, r, inv_index);
    m.fill(z, sdf, *beta_p);

    // ---- phase 2: weights, depth sums and the level candidates
    const bool out0 = live && lane == 0;
    float d_all = 0.f;
    float m_te = FLT_MAX, m_n = FLT_MAX, m_i = FLT_MAX, m_d = 0.f;      // this lane's merged candidate, key (te, person, sample)
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        if (p >= P) continue;
        float d_p = 0.f, a_s = 0.f, d_s = 0.f, lvl = -1.f;
        if (m.k[p] >= 0) {
            const float* te_l = m.te(p);
            const float* fe_l = m.fe(p);
            const float* pf_l = m.pf(p);
            const float t0 = z[p][(size_t)m.k[p] * n_z];
            float s_te = FLT_MAX, s_i = FLT_MAX, s_d = 0.f;              // this lane's solo candidate, key (te, sample)
            for (int i0 = 0; i0 < S; i0 += 64) {
                const int i = i0 + lane;
                if (i < S) {
                    const float te = te_l[i], fe = fe_l[i];
                    const float ts = i > 0 ? te_l[i - 1] : t0;
                    const float Es = pf_l[i];
                    const float E = m.energy_in_front(p, i);
                    const float a = 1.0f - expf(-fe);
                    const float tm = 0.5f * (ts + te);
                    const float w = a * expf(-E), ws = a * expf(-Es);
                    d_p += w * tm;
                    a_s += ws;
                    d_s += ws * tm;
                    if (E + fe >= L && te < m_te) {        // persons and samples ascend within a lane: strict < keeps the lower (n, i)
                        m_te = te; m_n = (float)p; m_i = (float)i; m_d = level_depth(ts, te, E, fe, L);
                    }
                    if (Es + fe >= L && te < s_te) {
                        s_te = te; s_i = (float)i; s_d = level_depth(ts, te, Es, fe, L);
                    }
                }
            }
            d_all += d_p;
            d_p = mp::wsum(d_p);
            a_s = mp::wsum(a_s);
            d_s = mp::wsum(d_s);
            const float b_te = mp::wmin(s_te);
            if (b_te < FLT_MAX) {
                const float b_i = mp::wmin(s_te == b_te ? s_i : FLT_MAX);
                lvl = mp::wmin(s_te == b_te && s_i == b_i ? s_d : FLT_MAX);
            }
        }
        if (out0) {
            const size_t o = (size_t)r * P + p;
            if (depth_person) depth_person[o] = d_p;
            if (acc_solo) acc_solo[o] = a_s;
            if (depth_solo) depth_solo[o] = d_s;
            if (depth_solo_level) depth_solo_level[o] = lvl;
        }
    }
    d_all = mp::wsum(d_all);
    float lvl = -1.f;
    int front = -1;
    const float b_te = mp::wmin(m_te);
    if (b_te < FLT_MAX) {
        const float b_n = mp::wmin(m_te == b_te ? m_n : FLT_MAX);
        const bool own = m_te == b_te && m_n == b_n;
        const float b_i = mp::wmin(own ? m_i : FLT_MAX);
        lvl = mp::wmin(own && m_i == b_i ? m_d : FLT_MAX);
        front = (int)b_n;
    }
    if (!out0) return;
    if (depth) depth[r] = d_all;
    if (depth_level) depth_level[r] = lvl;
    if (front_person) front_person[r] = front;
}

// ---- compositing backward: with dw = dC . rgb + dA + dA_p, the adjoint of fe_j is
//     dw_j T_j exp(-fe_j)  -  sum_{i behind j} dw_i w_i  -  [j is not the very last sample] dT_bg T_bg
// E and the sum behind are per-person prefix sums looked up at the ranks.  (The first version walked the merged list with one
// THREAD per ray: 512 threads on the whole device, ~1 ms.)
// DET (the deterministic form): d_beta is a buffer [n_rays] that receives every ray's own sum; k_beta_finish adds them in order.
template <bool DET = false>
__global__ __launch_bounds__(256) void k_composite_bwd(
    int n_rays, int P, int n_z, const int* const* __restrict__ inv_index, const float* const* __restrict__ z,
    const float* const* __restrict__ sdf, const float* const* __restrict__ rgb, const float* __restrict__ beta_p,
    const float* __restrict__ bg_rgb, const float* __restrict__ d_rgb_values, const float* __restrict__ d_acc,
    const float* __restrict__ d_acc_person, float* const* __restrict__ d_sdf, float* const* __restrict__ d_rgb,
    float* __restrict__ d_bg_rgb, float* __restrict__ d_beta) {
    extern __shared__ float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const int r = blockIdx.x * wpb + wave;
    const int S = n_z - 1;
    const float beta = *beta_p;
    const bool live = r < n_rays;
    const RayMerge m(smem, wave, S, bwd_stride(S), P, live, r, inv_index);   // extras: 0 gp [S+1] (prefix of dw w), 1 w [S]
    float dC[3] = {0.f, 0.f, 0.f}, dA = 0.f;
    if (live) {
        for (int a = 0; a < 3; ++a) dC[a] = d_rgb_values[3 * r + a];
        dA = d_acc ? d_acc[r] : 0.0f;
    }
    m.fill(z, sdf, beta);
    // ---- phase 2: weights, dw w and its per-person prefix sums
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        if (m.has(p)) {
            const float* fe_l = m.fe(p);
            float* gp_l = m.extra(p, 0);
            float* w_l = m.extra(p, 1);
            const float dAp = d_acc_person ? d_acc_person[(size_t)r * P + p] : 0.0f;
            float carry = 0.f;
            if (lane == 0) gp_l[0] = 0.f;
            for (int i0 = 0; i0 < S; i0 += 64) {
                const int i = i0 + lane;
                float g = 0.f;
                if (i < S) {
                    const float T = expf(-m.energy_in_front(p, i));
                    const float w = (1.0f - expf(-fe_l[i])) * T;
                    const size_t qi = (size_t)m.k[p] * S + i;
                    const float dw = dC[0] * rgb[p][3 * qi] + dC[1] * rgb[p][3 * qi + 1] + dC[2] * rgb[p][3 * qi + 2] + dA + dAp;
                    w_l[i] = w;
                    g = dw * w;
                    d_rgb[p][3 * qi] = w * dC[0]; d_rgb[p][3 * qi + 1] = w * dC[1]; d_rgb[p][3 * qi + 2] = w * dC[2];
                }
                float tot;
                const float ex = mp::wave_excl_scan(g, tot);
                if (i < S) gp_l[i + 1] = carry + ex + g;
                carry += tot;
            }
        }
    }
    __syncthreads();
    float Tbg;
    const int p_last = m.last_sample(Tbg);
    float dTbg = 0.f;
    for (int a = 0; a < 3; ++a) dTbg += dC[a] * (bg_rgb && live ? bg_rgb[3 * r + a] : 1.0f);
    if (live && lane < 3 && d_bg_rgb) d_bg_rgb[3 * r + lane] = dC[lane] * Tbg;
    // ---- phase 3: adjoints of the free energies -> sdf and beta
    float dbeta_local = 0.0f;
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        if (m.has(p)) {
            const float* te_l = m.te(p);
            const float* fe_l = m.fe(p);
            const float* pf_l = m.pf(p);
            const float* gp_l = m.extra(p, 0);
            const float* zr = z[p] + (size_t)m.k[p] * n_z;
            for (int i = lane; i < S; i += 64) {
                const float te = te_l[i], fe = fe_l[i];
                float E = pf_l[i], suffix = gp_l[S] - gp_l[i + 1];     // free energy in front, dw w behind
                m.others_in_front(p, te, [&](int q, int lo) {
                    E += m.pf(q)[lo];
                    suffix += m.extra(q, 0)[S] - m.extra(q, 0)[lo];
                });
                const float T = expf(-E), ex = expf(-fe);
                const size_t qi = (size_t)m.k[p] * S + i;
                const float dw = dC[0] * rgb[p][3 * qi] + dC[1] * rgb[p][3 * qi + 1] + dC[2] * rgb[p][3 * qi + 2] + dA +
                                 (d_acc_person ? d_acc_person[(size_t)r * P + p] : 0.0f);
                float dfe = dw * T * ex - suffix;
                if (!(p == p_last && i == S - 1)) dfe -= dTbg * Tbg;   // T_bg depends on every sample but the last
                const float dsig = dfe * (te - zr[i]);
                float dsdf, dbe;
                mp::laplace_density_adjoint(sdf[p][qi], beta, dsdf, dbe);
                d_sdf[p][qi] = dsig * dsdf;
                dbeta_local += dsig * dbe;
            }
        }
    }
    dbeta_local = mp::wsum(dbeta_local);
    if constexpr (DET) {
        if (lane == 0 && live) d_beta[r] = dbeta_local;
        return;
    }
    if (lane == 0 && dbeta_local != 0.0f) atomicAdd(d_beta, dbeta_local);
}

// ---- adjoint of the geometry outputs: d depth / d depth_person (merged sums of w tm), d acc_solo / d depth_solo (the person's
// own list: E = its own prefix sum) and d depth_solo_level.  Phase 2 fills TWO per-person prefix arrays (dw w in merged order,
// dws w0 in the person's own order) and finds the person's crossing sample j* by the forward's rule (minimum of (te, sample) over
// the samples with Es + fe >= L); phase 3 turns
//     dfe_j = dw_j e^-E e^-fe - sum_{behind j, merged} dw w  +  dws_j e^-Es e^-fe - sum_{i>j, own} dws w0  -  c [j < j*]  -  c f [j == j*]
// (c = d level (te-ts)/fe of sample j*, f = (L-Es)/fe there; nothing where the forward clamps or finds no crossing) into d sdf and
// d beta.  It ACCUMULATES (d_sdf +=: each element belongs to one lane), after k_composite_bwd's `=` on the same stream.
template <bool DET = false>       // DET: as k_composite_bwd
__global__ __launch_bounds__(256) void k_composite_geometry_bwd(
    int n_rays, int P, int n_z, const int* const* __restrict__ inv_index, const float* const* __restrict__ z,
    const float* const* __restrict__ sdf, const float* __restrict__ beta_p, float L, const float* __restrict__ d_depth,
    const float* __restrict__ d_depth_person, const float* __restrict__ d_acc_solo, const float* __restrict__ d_depth_solo,
    const float* __restrict__ d_depth_solo_level, float* const* __restrict__ d_sdf, float* __restrict__ d_beta) {
    extern __shared__ float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, wpb = blockDim.x >> 6;
    const int r = blockIdx.x * wpb + wave;
    const int S = n_z - 1;
    const float beta = *beta_p;
    const bool live = r < n_rays;
    const bool merged = d_depth || d_depth_person;          // (uniform) without them no rank is looked up
    // extras: 0 gm [S+1] (prefix of dw w), 1 gs [S+1] (prefix of dws w0)
    const RayMerge m(smem, wave, S, geometry_bwd_stride(S), P, live, r, inv_index);
    const float dD = (live && d_depth) ? d_depth[r] : 0.0f;
    m.fill(z, sdf, beta);
    // ---- phase 2: dw w (merged) and dws w0 (solo) with their prefix sums; the person's crossing sample
    float dwm[MAX_P], dAs[MAX_P], dDs[MAX_P], lc[MAX_P], lf[MAX_P];
    int jst[MAX_P];
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        dwm[p] = dAs[p] = dDs[p] = lc[p] = lf[p] = 0.0f;
        jst[p] = -1;
        if (m.has(p)) {
            const float* te_l = m.te(p);
            const float* fe_l = m.fe(p);
            const float* pf_l = m.pf(p);
            float* gm_l = m.extra(p, 0);
            float* gs_l = m.extra(p, 1);
            const size_t o = (size_t)r * P + p;
            const float t0 = z[p][(size_t)m.k[p] * n_z];
            dwm[p] = dD + (d_depth_person ? d_depth_person[o] : 0.0f);
            dAs[p] = d_acc_solo ? d_acc_solo[o] : 0.0f;
            dDs[p] = d_depth_solo ? d_depth_solo[o] : 0.0f;
            float carry_m = 0.f, carry_s = 0.f;
            if (lane == 0) gm_l[0] = gs_l[0] = 0.f;
            float s_te = FLT_MAX, s_i = FLT_MAX;               // this lane's solo candidate, key (te, sample)
            for (int i0 = 0; i0 < S; i0 += 64) {
                const int i = i0 + lane;
                float gm = 0.f, gs = 0.f;
                if (i < S) {
                    const float te = te_l[i], fe = fe_l[i];
                    const float ts = i > 0 ? te_l[i - 1] : t0;
                    const float Es = pf_l[i];
                    const float a = 1.0f - expf(-fe), tm = 0.5f * (ts + te);
                    if (merged) gm = dwm[p] * tm * a * expf(-m.energy_in_front(p, i));
                    gs = (dAs[p] + dDs[p] * tm) * a * expf(-Es);
                    if (Es + fe >= L && te < s_te) { s_te = te; s_i = (float)i; }
                }
                float tot;
                float ex = mp::wave_excl_scan(gm, tot);
                if (i < S) gm_l[i + 1] = carry_m + ex + gm;
                carry_m += tot;
                ex = mp::wave_excl_scan(gs, tot);
                if (i < S) gs_l[i + 1] = carry_s + ex + gs;
                carry_s += tot;
            }
            const float g = d_depth_solo_level ? d_depth_solo_level[o] : 0.0f;
            const float b_te = mp::wmin(s_te);
            if (g != 0.0f && b_te < FLT_MAX) {
                const int j = (int)mp::wmin(s_te == b_te ? s_i : FLT_MAX);
                const float fe = fe_l[j];
                const float f = fe > 0.f ? (L - pf_l[j]) / fe : 0.f;
                if (f > 0.f && f < 1.f) {
                    jst[p] = j;
                    lc[p] = g * (te_l[j] - (j > 0 ? te_l[j - 1] : t0)) / fe;
                    lf[p] = f;
                }
            }
        }
    }
    __syncthreads();
    // ---- phase 3: adjoints of the free energies -> sdf and beta
    float dbeta_local = 0.0f;
#pragma unroll
    for (int p = 0; p < MAX_P; ++p) {
        if (m.has(p)) {
            const float* te_l = m.te(p);
            const float* fe_l = m.fe(p);
            const float* pf_l = m.pf(p);
            const float* gm_l = m.extra(p, 0);
            const float* gs_l = m.extra(p, 1);
            const float* zr = z[p] + (size_t)m.k[p] * n_z;
            for (int i = lane; i < S; i += 64) {
                const float te = te_l[i], fe = fe_l[i], ts = zr[i];
                const float Es = pf_l[i], ex = expf(-fe), tm = 0.5f * (ts + te);
                float dfe = (dAs[p] + dDs[p] * tm) * expf(-Es) * ex - (gs_l[S] - gs_l[i + 1]);
                if (merged) {
                    float E = Es, suffix = gm_l[S] - gm_l[i + 1];      // free energy in front, dw w behind
                    m.others_in_front(p, te, [&](int q, int lo) {
                        E += m.pf(q)[lo];
                        suffix += m.extra(q, 0)[S] - m.extra(q, 0)[lo];
                    });
                    dfe += dwm[p] * tm * expf(-E) * ex - suffix;
                }
                if (i < jst[p]) dfe -= lc[p];
                else if (i == jst[p]) dfe -= lc[p] * lf[p];
                const size_t qi = (size_t)m.k[p] * S + i;
                const float dsig = dfe * (te - ts);
                float dsdf, dbe;
                mp::laplace_density_adjoint(sdf[p][qi], beta, dsdf, dbe);
                d_sdf[p][qi] += dsig * dsdf;
                dbeta_local += dsig * dbe;
            }
        }
    }
    dbeta_local = mp::wsum(dbeta_local);
    if constexpr (DET) {
        if (lane == 0 && live) d_beta[r] = dbeta_local;
        return;
    }
    if (lane == 0 && dbeta_local != 0.0f) atomicAdd(d_beta, dbeta_local);
}

// *out += part[0] + part[1] + .. in a fixed order: thread t adds part[t], part[t + 256], .. ascending, thread 0 the 256 sums ascending
__global__ __launch_bounds__(256) void k_beta_finish(const float* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float v = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) v += part[i];
    red[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 256; ++i) t += red[i];
        *out += t;
    }
}

// Launch shape of the family for `per_person` floats of LDS per person and wave.  rc -1: n_person outside [0, MAX_P]; rc -2: the
// block does not fit 160 KiB of LDS.  A fixed shape has WPB waves per block; an adaptive one halves them, down to one, until
// they fit.
struct LaunchShape { int rc, wpb, lds; };
LaunchShape launch_shape(int n_person, int per_person, bool adaptive) {
    if (n_person > MAX_P || n_person < 0) return {-1, 0, 0};
    const int per_wave = n_person * per_person * (int)sizeof(float);
    int wpb = WPB;
    while (adaptive && wpb > 1 && wpb * per_wave > LDS_MAX) wpb >>= 1;
    return {wpb * per_wave > LDS_MAX ? -2 : 0, wpb, wpb * per_wave};
}

}  // namespace

extern "C" int mp_composite(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                            const float* const* sdf, const float* const* rgb, const float* const* normal,
                            const float* beta, const float* bg_rgb, float* rgb_values, float* fg_rgb_values,
                            float* normal_values, float* acc_map, float* acc_person, float* bg_T, void* stream) {
    const LaunchShape sh = launch_shape(n_person, fwd_stride(n_z - 1), false);
    if (sh.rc == -1) return -1;
    if (n_rays <= 0) return 0;
    if (sh.rc) return sh.rc;
    MP_LDS_ATTR((k_composite), LDS_MAX);
    hipLaunchKernelGGL(k_composite, dim3((n_rays + WPB - 1) / WPB), dim3(64 * WPB), sh.lds, (hipStream_t)stream, n_rays, n_person,
                       n_z, inv_index, z, sdf, rgb, normal, beta, bg_rgb, rgb_values, fg_rgb_values, normal_values, acc_map,
                       acc_person, bg_T);
    return (int)hipGetLastError();
}

extern "C" int mp_composite_geometry(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                                     const float* const* sdf, const float* beta, float level, float* depth,
                                     float* depth_person, float* depth_level, int* front_person, float* acc_solo,
                                     float* depth_solo, float* depth_solo_level, void* stream) {
    const LaunchShape sh = launch_shape(n_person, fwd_stride(n_z - 1), false);
    if (sh.rc == -1) return -1;
    if (!(level > 0.f && level < 1.f)) return -3;
    if (n_rays <= 0) return 0;
    if (sh.rc) return sh.rc;
    MP_LDS_ATTR((k_composite_geometry), LDS_MAX);
    const float L = (float)-log1p(-(double)level);
    hipLaunchKernelGGL(k_composite_geometry, dim3((n_rays + WPB - 1) / WPB), dim3(64 * WPB), sh.lds, (hipStream_t)stream, n_rays,
                       n_person, n_z, inv_index, z, sdf, beta, L, depth, depth_person, depth_level, front_person, acc_solo,
                       depth_solo, depth_solo_level);
    return (int)hipGetLastError();
}

extern "C" int mp_tr_composite_bwd(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                                   const float* const* sdf, const float* const* rgb, const float* beta, const float* bg_rgb,
                                   const float* d_rgb_values, const float* d_acc, const float* d_acc_person,
                                   float* const* d_sdf, float* const* d_rgb, float* d_bg_rgb, float* d_beta, void* stream) {
    const LaunchShape sh = launch_shape(n_person, bwd_stride(n_z - 1), true);
    if (sh.rc == -1) return -1;
    if (n_rays <= 0) return 0;
    if (sh.rc) return sh.rc;
    MP_LDS_ATTR((k_composite_bwd<>), LDS_MAX);
    hipLaunchKernelGGL(k_composite_bwd<>, dim3((n_rays + sh.wpb - 1) / sh.wpb), dim3(64 * sh.wpb), sh.lds, (hipStream_t)stream, n_rays,
                       n_person, n_z, inv_index, z, sdf, rgb, beta, bg_rgb, d_rgb_values, d_acc, d_acc_person, d_sdf, d_rgb,
                       d_bg_rgb, d_beta);
    return (int)hipGetLastError();
}

extern "C" int mp_tr_composite_geometry_bwd(int n_rays, int n_person, int n_z, const int* const* inv_index,
                                            const float* const* z, const float* const* sdf, const float* beta, float level,
                                            const float* d_depth, const float* d_depth_person, const float* d_acc_solo,
                                            const float* d_depth_solo, const float* d_depth_solo_level, float* const* d_sdf,
                                            float* d_beta, void* stream) {
    const LaunchShape sh = launch_shape(n_person, geometry_bwd_stride(n_z - 1), true);
    if (sh.rc == -1) return -1;
    if (!(level > 0.f && level < 1.f)) return -3;
    if (n_rays <= 0) return 0;
    if (!d_depth && !d_depth_person && !d_acc_solo && !d_depth_solo && !d_depth_solo_level) return 0;
    if (sh.rc) return sh.rc;
    MP_LDS_ATTR((k_composite_geometry_bwd<>), LDS_MAX);
    const float L = (float)-log1p(-(double)level);
    hipLaunchKernelGGL(k_composite_geometry_bwd<>, dim3((n_rays + sh.wpb - 1) / sh.wpb), dim3(64 * sh.wpb), sh.lds, (hipStream_t)stream,
                       n_rays, n_person, n_z, inv_index, z, sdf, beta, L, d_depth, d_depth_person, d_acc_solo, d_depth_solo,
                       d_depth_solo_level, d_sdf, d_beta);
    return (int)hipGetLastError();
}

// Deterministic forms: d_beta_part [n_rays] is the caller's scratch for the rays' own sums (written, never read back by the caller)
extern "C" int mp_tr_composite_bwd_det(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                                       const float* const* sdf, const float* const* rgb, const float* beta, const float* bg_rgb,
                                       const float* d_rgb_values, const float* d_acc, const float* d_acc_person,
                                       float* const* d_sdf, float* const* d_rgb, float* d_bg_rgb, float* d_beta,
                                       float* d_beta_part, void* stream) {
    const LaunchShape sh = launch_shape(n_person, bwd_stride(n_z - 1), true);
    if (sh.rc == -1) return -1;
    if (n_rays <= 0) return 0;
    if (sh.rc) return sh.rc;
    if (d_beta_part == nullptr) return -3;
    MP_LDS_ATTR((k_composite_bwd<true>), LDS_MAX);
    hipLaunchKernelGGL(k_composite_bwd<true>, dim3((n_rays + sh.wpb - 1) / sh.wpb), dim3(64 * sh.wpb), sh.lds, (hipStream_t)stream,
                       n_rays, n_person, n_z, inv_index, z, sdf, rgb, beta, bg_rgb, d_rgb_values, d_acc, d_acc_person, d_sdf, d_rgb,
                       d_bg_rgb, d_beta_part);
    hipLaunchKernelGGL(k_beta_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, d_beta_part, n_rays, d_beta);
    return (int)hipGetLastError();
}

extern "C" int mp_tr_composite_geometry_bwd_det(int n_rays, int n_person, int n_z, const int* const* inv_index,
                                                const float* const* z, const float* const* sdf, const float* beta, float level,
                                                const float* d_depth, const float* d_depth_person, const float* d_acc_solo,
                                                const float* d_depth_solo, const float* d_depth_solo_level, float* const* d_sdf,
                                                float* d_beta, float* d_beta_part, void* stream) {
    const LaunchShape sh = launch_shape(n_person, geometry_bwd_stride(n_z - 1), true);
    if (sh.rc == -1) return -1;
    if (!(level > 0.f && level < 1.f)) return -3;
    if (n_rays <= 0) return 0;
    if (!d_depth && !d_depth_person && !d_acc_solo && !d_depth_solo && !d_depth_solo_level) return 0;
    if (sh.rc) return sh.rc;
    if (d_beta_part == nullptr) return -3;
    MP_LDS_ATTR((k_composite_geometry_bwd<true>), LDS_MAX);
    const float L = (float)-log1p(-(double)level);
    hipLaunchKernelGGL(k_composite_geometry_bwd<true>, dim3((n_rays + sh.wpb - 1) / sh.wpb), dim3(64 * sh.wpb), sh.lds,
                       (hipStream_t)stream, n_rays, n_person, n_z, inv_index, z, sdf, beta, L, d_depth, d_depth_person, d_acc_solo,
                       d_depth_solo, d_depth_solo_level, d_sdf, d_beta_part);
    hipLaunchKernelGGL(k_beta_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, d_beta_part, n_rays, d_beta);
    return (int)hipGetLastError();
}
