// The exact nearest-vertex search on a clustered vertex set in LDS (mp_knn_build's tables): shared by the warp kernels
// (geom.hip) and the cross-person probe of the interpenetration term (penetration.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"

typedef float f32x2 __attribute__((ext_vector_type(2)));

// cycle / event counters of the warp kernels (-DMP_GEOM_PROF, geom.hip defines them before this header); no-ops elsewhere
#ifndef GP_T
#define GP_T() 0ull
#define GP_ADD(i, v) do { } while (0)
#define GP_BEGIN() do { } while (0)
#define GP_END() do { } while (0)
#endif

namespace {

// Exact nearest vertex among the clustered set held in LDS (vs, cb), for the 64 points of one wave at once.
// The wave's points are spatially coherent (neighbouring rays at the same sample index), so clusters are culled ONCE per
// wave against the bounding box of its points: lane c tests clusters c and c+64 in parallel (two LDS reads instead of a
// latency-bound loop over all the spheres), and only the surviving clusters are scanned vertex by vertex.
//   cap2 (per lane): squared search radius; < 0 = idle lane.  A vertex within the cap, if any, is the exact nearest one
//   (ties -> lowest vertex id, like an argmin over the original order: pytorch3d knn_points / deformer.py:39).
//   Returns bi = INT_MAX when no vertex lies within the cap.
//   NC / CL: the granularity searched (the fine clusters, or pairs of them: cb = the coarse spheres, see k_knn_build).
#ifndef MP_KNN_BP
#define MP_KNN_BP 2      // vertex pairs read ahead in the cluster scan
#endif
template <int NCX = MP_KNN_NC, int CLX = MP_KNN_CLUSTER>
__device__ __forceinline__ void knn_capped(const float4* vs, const float4* cb, float px, float py, float pz, float cap2,
                                           float& best, int& bi) {
    constexpr int NC = NCX, CL = CLX;
    const int lane = threadIdx.x & 63;
    const bool on = cap2 >= 0.0f;
    const unsigned long long gp0 = GP_T();
    const float lx = mp::wmin(on ? px : FLT_MAX), ly = mp::wmin(on ? py : FLT_MAX), lz = mp::wmin(on ? pz : FLT_MAX);
    const float hx = mp::wmax(on ? px : -FLT_MAX), hy = mp::wmax(on ? py : -FLT_MAX), hz = mp::wmax(on ? pz : -FLT_MAX);
    const float capr = sqrtf(mp::wmax(on ? cap2 : 0.0f));
    constexpr int NH = (NC + 63) / 64;      // candidate masks: 64 clusters each
    unsigned long long cand[NH];
    // the candidate sphere closest to the middle of the wave's points is scanned first: it usually holds the neighbour of
    // most lanes, and with that distance in hand the per-cluster bound below rejects most of the other candidates
    const float mx = 0.5f * (lx + hx), my = 0.5f * (ly + hy), mz = 0.5f * (lz + hz);
    float nearest = FLT_MAX;
    int nearest_c = -1;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int c = lane + 64 * h;
        bool hit = false;
        if (c < NC) {
            const float4 b = cb[c];
            const float dx = b.x - fminf(fmaxf(b.x, lx), hx), dy = b.y - fminf(fmaxf(b.y, ly), hy),
                        dz = b.z - fminf(fmaxf(b.z, lz), hz);
            const float reach = (b.w + capr) * 1.0001f;
            hit = dx * dx + dy * dy + dz * dz <= reach * reach;
            const float ex = b.x - mx, ey = b.y - my, ez = b.z - mz;
            const float gap = sqrtf(ex * ex + ey * ey + ez * ez) - b.w;
            if (hit && gap < nearest) { nearest = gap; nearest_c = c; }
        }
        cand[h] = __ballot(hit);
    }
    int first_c = -1;
    unsigned long long any_c = 0;
#pragma unroll
    for (int h = 0; h < NH; ++h) any_c |= cand[h];
    if (any_c) {
        const float wm = mp::wmin(nearest);
        const unsigned long long who = __ballot(nearest_c >= 0 && nearest == wm);
        first_c = __shfl(nearest_c, __builtin_ctzll(who));
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (h == (first_c >> 6)) cand[h] &= ~(1ull << (first_c & 63));
    }
    // running minimum as ONE 64-bit key (distance bits << 32 | vertex id): distances are >= 0, so their bit patterns order
    // like the values, and a tie in distance falls through to the lower vertex id (the argmin order of the reference's
    // brute-force search) -- one v_cmp_lt_u64 and two selects per vertex, no branch in the scan.  Lanes that are off
    // hold key 0, which nothing undercuts.  [Round 6 tried (distance, id) with a FLOAT compare + a wave-wide tie mask that
    // repeats the search with these keys when a distance equals a running minimum: 14 instead of 16 VALU instructions per
    // vertex pair, and SLOWER (training warp 64 -> 79 us, sampler warp 2.24 -> 2.34 ms): the compares then write scalar
    // mask pairs (VOP3) that the selects read back behind wait states.  tests/test_geom_gpu.py holds the tie test it left.]
    unsigned long long key = on ? (((unsigned long long)__float_as_uint(cap2) << 32) | (unsigned)INT_MAX) : 0ull;
    const f32x2 PX = {px, px}, PY = {py, py}, PZ = {pz, pz};
    const unsigned long long gp1 = GP_T();
    GP_ADD(2, gp1 - gp0);
#pragma unroll
    for (int h = 0; h < NH; ++h) GP_ADD(4, __popcll(cand[h]));
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        unsigned long long m = cand[h];
        while (m || (h == 0 && first_c >= 0)) {
            int c;
            if (h == 0 && first_c >= 0) { c = first_c; first_c = -1; }
            else { c = __builtin_ctzll(m) + 64 * h; m &= m - 1; }
            const float4 b = cb[c];
            const float ex = px - b.x, ey = py - b.y, ez = pz - b.z;
            const float lb = fmaxf(sqrtf(ex * ex + ey * ey + ez * ez) - b.w, 0.0f);
            if (!__any(on && lb * lb * 0.9999f <= __uint_as_float((unsigned)(key >> 32)))) continue;   // no lane can improve here
            GP_ADD(5, 1);
            // two vertices per step in packed fp32 (v_pk_add / v_pk_mul / v_pk_fma_f32): the cluster is stored as pairs
            // (xa xb ya yb)(za zb ida idb), see load_knn_lds
            // The reads are software-pipelined by hand, KNN_BP pairs ahead (round 6): left to itself the compiler issued the two
            // reads of a pair and waited for them at once -- hidden by the other waves of an eval launch, but a training launch has
            // ONE wave per SIMD and paid the LDS latency 32 times per cluster (6.4 k cycles per 64 vertices, tools/geom_prof_train.py).
            const float4* cv = vs + c * CL;
            constexpr int BP = MP_KNN_BP;
            static_assert((CL / 2) % BP == 0, "pairs per block");
            float4 A[BP], B[BP], An[BP], Bn[BP];
#pragma unroll
            for (int j = 0; j < BP; ++j) { A[j] = cv[2 * j]; B[j] = cv[2 * j + 1]; }
#pragma unroll
            for (int k0 = 0; k0 < CL / 2; k0 += BP) {
                if (k0 + BP < CL / 2) {
#pragma unroll
                    for (int j = 0; j < BP; ++j) { An[j] = cv[2 * (k0 + BP + j)]; Bn[j] = cv[2 * (k0 + BP + j) + 1]; }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < BP; ++j) {
                    const f32x2 fx = PX - (f32x2){A[j].x, A[j].y}, fy = PY - (f32x2){A[j].z, A[j].w}, fz = PZ - (f32x2){B[j].x, B[j].y};
                    const f32x2 d2 = __builtin_elementwise_fma(fz, fz, __builtin_elementwise_fma(fy, fy, fx * fx));
                    const unsigned long long ka = ((unsigned long long)__float_as_uint(d2.x) << 32) | __float_as_uint(B[j].z);
                    const unsigned long long kb = ((unsigned long long)__float_as_uint(d2.y) << 32) | __float_as_uint(B[j].w);
                    key = ka < key ? ka : key;
                    key = kb < key ? kb : key;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < BP; ++j) { A[j] = An[j]; B[j] = Bn[j]; }
            }
        }
    }
    best = on ? __uint_as_float((unsigned)(key >> 32)) : cap2;
    bi = on ? (int)(unsigned)(key & 0xffffffffull) : INT_MAX;
    GP_ADD(3, GP_T() - gp1);
}

// the fine clusters and their spheres, global -> LDS (vs [MP_KNN_NC * MP_KNN_CLUSTER], cb [MP_KNN_NC])
__device__ __forceinline__ void load_knn_lds(float4* vs, float4* cb, const float* vsorted, const float* cbound) {
    constexpr int NC = MP_KNN_NC, CL = MP_KNN_CLUSTER;
    const float4* gv = (const float4*)vsorted;
    const float4* gc = (const float4*)cbound;
    for (int i = threadIdx.x; i < NC * CL / 2; i += blockDim.x) {      // vertex pair (2i, 2i+1) -> (xa xb ya yb)(za zb ida idb)
        const float4 a = gv[2 * i], b = gv[2 * i + 1];
        vs[2 * i] = make_float4(a.x, b.x, a.y, b.y);
        vs[2 * i + 1] = make_float4(a.z, b.z, a.w, b.w);
    }
    for (int i = threadIdx.x; i < NC; i += blockDim.x) cb[i] = gc[i];
}

}  // namespace
