// One wave's view of the merge of its ray's per-person sample lists: the core of the four compositing kernels (composite.hip).
// Each person's samples are already sorted by t_end, so "in front of sample (p, i) in the merged order" needs no merge: it is
// person p's own samples before i plus, for every other person q, the first rank(q, p, t_end(p, i)) samples of q.  Per person
// the wave keeps in LDS
//     te [S] (t_end) | fe [S] (free energy sigma dt) | pf [S+1] (exclusive prefix sums of fe, pf[0] = 0) | the kernel's extras
// and every sum over "the samples in front" is a prefix array looked up at those ranks.
#pragma once
#include <float.h>
#include "common.hpp"

namespace mp {

constexpr int MAX_P = 8;   // persons per ray

struct RayMerge {
    float* base;     // this wave's LDS
    int S, stride;   // samples per person; floats per person: prefix_floats(S) + the kernel's extras
    int P;
    int k[MAX_P];    // the ray's row in person p's arrays; -1: dead wave, missed person, p >= P

    static constexpr int prefix_floats(int S) { return 3 * S + 1; }

    __device__ __forceinline__ RayMerge(float* smem, int wave, int S_, int stride_, int P_, bool live, int r,
                                        const int* const* __restrict__ inv_index)
        : base(smem + (size_t)wave * P_ * stride_), S(S_), stride(stride_), P(P_) {
#pragma unroll
        for (int p = 0; p < MAX_P; ++p) k[p] = (live && p < P) ? inv_index[p][r] : -1;
    }

    // person p hits the ray.  k[p] says it all: a test of p < P on top costs k_composite 22 SGPRs and a wave per SIMD
    // (profiles/composite_merge.txt)
    __device__ __forceinline__ bool has(int p) const { return k[p] >= 0; }
    __device__ __forceinline__ float* te(int p) const { return base + p * stride; }
    __device__ __forceinline__ float* fe(int p) const { return te(p) + S; }
    __device__ __forceinline__ float* pf(int p) const { return te(p) + 2 * S; }
    // the n-th array behind the prefix; extras are laid out S+1 floats apart (the last one may be S long)
    __device__ __forceinline__ float* extra(int p, int n) const { return pf(p) + (n + 1) * (S + 1); }

    // phase 1: te, fe and pf of every person that hits the ray; the block may read them on return
    __device__ __forceinline__ void fill(const float* const* __restrict__ z, const float* const* __restrict__ sdf, float beta) const {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int p = 0; p < MAX_P; ++p) {
            if (has(p)) {
                float* te_l = te(p);
                float* fe_l = fe(p);
                float* pf_l = pf(p);
                const float* zr = z[p] + (size_t)k[p] * (S + 1);
                const float* sr = sdf[p] + (size_t)k[p] * S;
                float carry = 0.f;
                if (lane == 0) pf_l[0] = 0.f;
                for (int i0 = 0; i0 < S; i0 += 64) {
                    const int i = i0 + lane;
                    float f = 0.f;
                    if (i < S) {
                        const float ts = zr[i], t = zr[i + 1];
                        f = laplace_density(sr[i], beta) * (t - ts);
                        te_l[i] = t;
                        fe_l[i] = f;
                    }
                    float tot;
                    const float ex = wave_excl_scan(f, tot);
                    if (i < S) pf_l[i + 1] = carry + ex + f;
                    carry += tot;
                }
            }
        }
        __syncthreads();
    }

    // number of q's samples in front of a sample of person p (q != p) that ends at t: t_end < t, or <= t for q < p (ties: the
    // lower person first, the order of the reference's stable sorts)
    __device__ __forceinline__ int rank(int q, int p, float t) const {
        const float* te_q = te(q);
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const float v = te_q[mid];
            const bool before = q < p ? v <= t : v < t;
            if (before) lo = mid + 1; else hi = mid;
        }
        return lo;
    }

    // f(q, rank) for every other live person q: rank = the number of q's samples in front of a sample of person p that ends at t
    template <class F>
    __device__ __forceinline__ void others_in_front(int p, float t, F f) const {
#pragma unroll
        for (int q = 0; q < MAX_P; ++q)
            if (q != p && has(q)) f(q, rank(q, p, t));
    }

    // free energy in front of sample (p, i) in the merged order
    __device__ __forceinline__ float energy_in_front(int p, int i) const {
        float E = pf(p)[i];
        others_in_front(p, te(p)[i], [&](int q, int lo) { E += pf(q)[lo]; });
        return E;
    }

    // the very last sample of the merged order (multiply.py:457-463) is the last sample of the person whose final t_end is the
    // largest (ties: the higher person).  -> that person, -1 for a ray without samples; T_front: the exclusive transmittance of
    // that sample (everything of the other persons and the person's own first S-1), 1 without samples
    __device__ __forceinline__ int last_sample(float& T_front) const {
        int p_last = -1;
        float tm = -FLT_MAX;
#pragma unroll
        for (int p = 0; p < MAX_P; ++p)
            if (has(p) && te(p)[S - 1] >= tm) { tm = te(p)[S - 1]; p_last = p; }
        float E_front = 0.f;
#pragma unroll
        for (int p = 0; p < MAX_P; ++p)
            if (has(p)) E_front += pf(p)[p == p_last ? S - 1 : S];
        T_front = p_last >= 0 ? expf(-E_front) : 1.0f;
        return p_last;
    }
};

}  // namespace mp
