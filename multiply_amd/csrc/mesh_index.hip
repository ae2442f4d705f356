// Face index for the exact mesh signed distance: mp_mesh_index_signed_distance returns, bit for bit, what the brute-force
// mp_mesh_signed_distance (mesh.hip) returns, without visiting the faces that cannot matter.  Both kernels evaluate a face with
// the same tri_dist2 / ray_x_crosses (mesh_prims.hpp); the minimum over faces and the parity of the crossings do not depend on the
// order of the faces, so the result is equal as long as no skipped face could have lowered the minimum or crossed the ray.
// The same index answers the closest-face query (mp_mesh_index_closest = the bits of mp_mesh_closest, mesh_closest.hip) with a
// kernel and a primitive of its own, k_index_closest and tri_closest; the signed path does not share arithmetic with it.
//
// The index is an implicit complete binary tree of axis-aligned boxes over the faces in Hilbert-curve order of their centroids:
//   leaf l  = faces 8 l .. 8 l + 7 of the sorted list (the last leaf may be partial), NL = ceil(F / 8) leaves;
//   NLp     = NL rounded up to a power of two; the leaves beyond NL are empty: lo = +inf, hi = -inf, no faces;
//   node i  (heap layout: root 1, children 2 i and 2 i + 1, leaf l = node NLp + l) = exact min / max of the vertex
//             coordinates below it, filled bottom-up.
// Buffer (mp_mesh_index_bytes, 16-byte aligned):  [16 floats: box of all vertices, lo at 0..2, hi at 4..6]
//   [2 NLp nodes x 8 floats: lo.xyz, -, hi.xyz, -; node 0 unused]  [8 NL faces x 9 floats, sorted order].
// Everything is built on the device: mp_mesh_index_keys (box reduction + curve keys) -> a sort of the keys by the caller ->
// mp_mesh_index_build (gather, leaf boxes, inner levels).  No host synchronisation anywhere.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include "../../include/multiply_hip.h"
#include "mesh_prims.hpp"

namespace {

constexpr int LEAF = 8;                 // faces per leaf
constexpr int HDR_FLOATS = 16;
constexpr int QB = 64;                  // points per workgroup of the query: one wave, so that a slow walk holds up 63 others at most
constexpr int TOP = 256;                // the levels of at most TOP nodes are filled by one workgroup

__host__ __device__ inline int n_leaves(int F) { return (F + LEAF - 1) / LEAF; }
__host__ __device__ inline int n_leaves_pow2(int F) {
    int p = 1;
    while (p < n_leaves(F)) p <<= 1;
    return p;
}

// ---- build --------------------------------------------------------------------------------------------------------------
// box of all 3 F vertices, one workgroup (F ~ 10^4..10^5: a few hundred strided loads per thread)
__global__ __launch_bounds__(1024) void k_index_bbox(const float* __restrict__ fv, int F, float* __restrict__ hdr) {
    __shared__ float sh[6][1024];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = threadIdx.x; v < 3 * F; v += 1024)
        for (int a = 0; a < 3; ++a) {
            const float c = fv[3 * (size_t)v + a];
            lo[a] = fminf(lo[a], c);
            hi[a] = fmaxf(hi[a], c);
        }
    for (int a = 0; a < 3; ++a) { sh[a][threadIdx.x] = lo[a]; sh[3 + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; ++a) {
                sh[a][threadIdx.x] = fminf(sh[a][threadIdx.x], sh[a][threadIdx.x + s]);
                sh[3 + a][threadIdx.x] = fmaxf(sh[3 + a][threadIdx.x], sh[3 + a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) { hdr[threadIdx.x] = sh[threadIdx.x][0]; hdr[4 + threadIdx.x] = sh[3 + threadIdx.x][0]; }
}

__device__ __forceinline__ unsigned spread10(unsigned v) {   // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Hilbert key of the face centroid inside the box of all vertices: the cell (10 bits per axis) -> its position along the
// Hilbert curve (Skilling, "Programming the Hilbert curve", AIP Conf. Proc. 707, 2004: axes to transpose, then the bits
// interleaved).  Consecutive cells of that curve are neighbours, so 8 consecutive faces form a compact patch.  The Morton curve
// jumps, and a leaf across a jump gets a box that every point enters: on a 20 480-face sphere a point near the surface evaluated
// 330 faces in Morton order and 150 in this one.  An axis of zero extent (a planar mesh) gets cell 0: the scale is set to 0 there
// instead of dividing by the extent.
__device__ __forceinline__ unsigned curve_cell(float c, float lo, float hi) {
    const float ext = hi - lo;
    const float scale = ext > 0.f ? 1024.f / ext : 0.f;
    return (unsigned)(int)fminf(fmaxf((c - lo) * scale, 0.f), 1023.f);          // (NaN -> 0 by fmaxf)
}

__device__ __forceinline__ int hilbert_key(unsigned X[3]) {
    for (unsigned Q = 512; Q > 1; Q >>= 1) {
        const unsigned P = Q - 1;
        for (int a = 0; a < 3; ++a) {
            if (X[a] & Q) X[0] ^= P;
            else { const unsigned t = (X[0] ^ X[a]) & P; X[0] ^= t; X[a] ^= t; }
        }
    }
    X[1] ^= X[0];
    X[2] ^= X[1];
    unsigned t = 0;
    for (unsigned Q = 512; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    return (int)((spread10(X[0] ^ t) << 2) | (spread10(X[1] ^ t) << 1) | spread10(X[2] ^ t));
}

__global__ void k_index_keys(const float* __restrict__ fv, int F, const float* __restrict__ hdr, int* __restrict__ keys) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    unsigned X[3];
    for (int a = 0; a < 3; ++a) {
        const float c = (fv[9 * (size_t)f + a] + fv[9 * (size_t)f + 3 + a] + fv[9 * (size_t)f + 6 + a]) * (1.f / 3.f);
        X[a] = curve_cell(c, hdr[a], hdr[4 + a]);
    }
    keys[f] = hilbert_key(X);
}

// the same key for query points (mp_mesh_index_point_keys): points in key order walk the tree alike, so the lanes of a wave
// finish together.  Points outside the mesh's box fall into its border cells.
__global__ void k_index_point_keys(const float* __restrict__ pts, int n, const float* __restrict__ hdr, int* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned X[3];
    for (int a = 0; a < 3; ++a) X[a] = curve_cell(pts[3 * (size_t)i + a], hdr[a], hdr[4 + a]);
    keys[i] = hilbert_key(X);
}

// faces into sorted order and the leaf boxes: one thread per leaf (empty leaves included)
__global__ void k_index_leaves(const float* __restrict__ fv, int F, const long long* __restrict__ order, float* __restrict__ nodes,
                               float* __restrict__ faces) {
    const int NLp = n_leaves_pow2(F);
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= NLp) return;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = LEAF * l; k < min(LEAF * (l + 1), F); ++k) {
        const long long src = min(max(order[k], 0ll), (long long)F - 1);   // (a permutation by contract; never read outside fv)
        for (int e = 0; e < 9; ++e) {
            const float c = fv[9 * (size_t)src + e];
            faces[9 * (size_t)k + e] = c;
            lo[e % 3] = fminf(lo[e % 3], c);
            hi[e % 3] = fmaxf(hi[e % 3], c);
        }
    }
    float* nd = nodes + 8 * (size_t)(NLp + l);
    for (int a = 0; a < 3; ++a) { nd[a] = lo[a]; nd[4 + a] = hi[a]; }
    nd[3] = nd[7] = 0.f;
}

__device__ __forceinline__ void merge_children(float* nodes, int i) {
    const float* l = nodes + 8 * (size_t)(2 * i);
    const float* r = l + 8;
    float* nd = nodes + 8 * (size_t)i;
    for (int a = 0; a < 3; ++a) { nd[a] = fminf(l[a], r[a]); nd[4 + a] = fmaxf(l[4 + a], r[4 + a]); }
    nd[3] = nd[7] = 0.f;
}

// one level of n nodes (n a power of two: nodes n .. 2 n - 1) from the level below
__global__ void k_index_level(float* nodes, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) merge_children(nodes, n + t);
}

// the levels of n0 <= TOP, n0 / 2, .., 1 nodes in one workgroup (a barrier between levels orders the global writes and reads)
__global__ __launch_bounds__(TOP) void k_index_top(float* nodes, int n0) {
    for (int n = n0; n >= 1; n >>= 1) {
        if ((int)threadIdx.x < n) merge_children(nodes, n + threadIdx.x);
        __syncthreads();
    }
}

// ---- query --------------------------------------------------------------------------------------------------------------
// exact-arithmetic lower bound of the squared distance from p to anything inside the box, evaluated in fp32
__device__ __forceinline__ float box_dist2(const float* p, const float4 lo, const float4 hi) {
    const float dx = fmaxf(fmaxf(lo.x - p[0], p[0] - hi.x), 0.f);
    const float dy = fmaxf(fmaxf(lo.y - p[1], p[1] - hi.y), 0.f);
    const float dz = fmaxf(fmaxf(lo.z - p[2], p[2] - hi.z), 0.f);
    return dx * dx + dy * dy + dz * dz;
}

// One thread per point.  A greedy descent to one leaf, evaluated first, gives an upper bound of the distance, then a stackless
// depth-first walk in heap order: from node i the walk goes to 2 i when the node is entered and is not a leaf, and otherwise to
// the next node in pre-order that is not below i: (i + 1) >> ctz(i + 1) -- the sibling of the nearest ancestor-or-self that is a left child;
// that is 1 after the last node.  No stack in registers, scratch or LDS.  Every node is tested at most once (the seed leaf
// twice), and the loop is capped at that count besides.
__global__ __launch_bounds__(QB) void k_index_sdist(const float* __restrict__ pts, int n, const float* __restrict__ index, int F,
                                                    float* __restrict__ sdist, int* __restrict__ visits) {
    const int i = blockIdx.x * QB + threadIdx.x;
    if (i >= n) return;
    const int NLp = n_leaves_pow2(F);
    const float4* nodes = reinterpret_cast<const float4*>(index + HDR_FLOATS);
    const float* faces = index + HDR_FLOATS + 16 * (size_t)NLp;
    const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};

    // Slack of the distance test.  tri_dist2 returns |p - q|^2 for a point q = a + v ab + w ac that it forms in fp32: each
    // component of q, and of p - q after it, is rounded at the magnitude of the COORDINATES, not of the distance, so the value
    // can fall short of the true squared distance d^2 to the face by what an absolute error of a few ulp(M) per component makes,
    // M = the largest |coordinate| involved (< 8 u M in norm with u = 2^-24; barycentrics that rounding pushes out of [0, 1] move
    // q along the face's plane by the same order).  A face in a box at exact distance >= sqrt(lb) therefore returns at least
    // (sqrt(lb) - delta)^2 (1 - 4 u); it cannot lower `best` when lb > (sqrt(best) + delta)^2 (1 + 16 FLT_EPSILON) =: bound, with
    // delta = 16 FLT_EPSILON M = 32 u M taken four times larger than the estimate, and the factor covering the roundings of
    // lb, of the three squares and of `bound` itself.  M is taken over the point and the box of the whole mesh (the root).
    // Slivers, where va, vb, vc cancel and the barycentrics are ill-conditioned, stay inside that: on 8 10^7 random triangles,
    // half of them slivers down to an aspect of 1e-7, at offsets 0 and 50, the fp32 value fell short of a double-precision
    // reference by 2.1 FLT_EPSILON M at most.  A zero-area face returns NaN (0 / 0), which fminf drops here as in brute force.
    const float4 rlo = nodes[2], rhi = nodes[3];
    float M = fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
    M = fmaxf(M, fmaxf(fmaxf(fmaxf(fabsf(rlo.x), fabsf(rhi.x)), fmaxf(fabsf(rlo.y), fabsf(rhi.y))), fmaxf(fabsf(rlo.z), fabsf(rhi.z))));
    const float delta = 16.f * FLT_EPSILON * M;
    // Slack of the crossing test in z.  ray_x_crosses counts an edge (u, w) that straddles p.y when zc = u.z + t (w.z - u.z) > p.z,
    // t = (p.y - u.y) / (w.y - u.y).  |p.y - u.y| <= |w.y - u.y| holds after rounding too (rounding is monotone), so t lies in
    // [0, 1 + 3 u] whatever the divide's last bits, and zc lies between u.z and w.z up to the roundings of w.z - u.z, of the
    // product and of the sum: |error| < 12 u Mz, Mz = the largest |z| of the mesh.  16 u Mz = 8 FLT_EPSILON Mz is used.
    const float sz = 8.f * FLT_EPSILON * fmaxf(fabsf(rlo.z), fabsf(rhi.z));

    float best = FLT_MAX;
    int crossings = 0, nodes_tested = 0, faces_tested = 0;
    // seed: towards the nearer child until a leaf; the walk below starts at that leaf (for the distance only), then at the root
    int seed = 1;
    while (seed < NLp) {
        const float dl = box_dist2(p, nodes[4 * seed], nodes[4 * seed + 1]), dr = box_dist2(p, nodes[4 * seed + 2], nodes[4 * seed + 3]);
        seed = dr < dl ? 2 * seed + 1 : 2 * seed;
        nodes_tested += 2;
    }
    float bound = INFINITY;                // nothing is far before the first leaf
    bool seeding = true;
    int node = seed;
    for (int it = 0; it <= 2 * NLp; ++it) {
        const float4 lo = nodes[2 * node], hi = nodes[2 * node + 1];
        ++nodes_tested;
        // Non-finite points.  box_dist2 is no guard by itself: fmaxf drops a NaN, so a NaN axis counts as distance 0 and the sum
        // stays finite.  What keeps such a point equal to brute force is `bound`: tri_dist2 returns NaN or +inf for every face
        // when a coordinate of p is NaN or +-inf, fminf keeps best = FLT_MAX (as in k_mesh_sdist), and (sqrt(FLT_MAX) + delta)^2
        // (1 + 16 FLT_EPSILON) overflows to +inf -- as does the initial bound -- so `far` is never true and the result is
        // sqrt(FLT_MAX) either way.  Whoever changes how `bound` is seeded or updated has to keep that.  The crossing test skips a
        // node only on comparisons that are true: with a NaN p.y or p.z they are false and the column is walked; with a NaN p.x
        // the faces that are walked answer x > NaN = false, as every face does in brute force.
        const bool far = box_dist2(p, lo, hi) > bound;
        // Crossing.  An edge counts only if exactly one endpoint has y > p.y, an exact comparison: some vertex y <= p.y and some
        // vertex y > p.y, i.e. lo.y <= p.y < hi.y, with no slack (the half-open rule itself).  Above the box in z (p.z >= hi.z + sz)
        // no straddling edge can have zc > p.z: no crossing.  Below it (p.z < lo.z - sz) every straddling edge has, and a triangle
        // has 0 or 2 straddling edges: an even count, no crossing.  There is NO test in x: the plane's x at (p.y, p.z) is a
        // quotient by the normal's x component, and for a face seen edge-on from the ray that quotient is not bounded by the box
        // at any slack -- brute force counts whatever it rounds to, so the walk has to look at every face of the (y, z) column.
        const bool miss = seeding || p[1] < lo.y || p[1] >= hi.y || p[2] >= hi.z + sz || p[2] < lo.z - sz;
        if (!(far && miss)) {
            if (node < NLp) { node = 2 * node; continue; }
            // The ONE place where faces are evaluated, with both primitives side by side as in k_mesh_sdist's loop: the compiler
            // contracts and pairs the arithmetic of an inlined copy by its surroundings, and a copy of tri_dist2 standing alone
            // was seen to differ from brute force in the last bit.  What the node did not need is masked, not skipped.
            const int l = node - NLp;
            for (int k = LEAF * l; k < min(LEAF * (l + 1), F); ++k) {
                float a[9];
                for (int e = 0; e < 9; ++e) a[e] = faces[9 * (size_t)k + e];
                const float d2 = tri_dist2(p, a, a + 3, a + 6);
                const int c = ray_x_crosses(p, a, a + 3, a + 6) ? 1 : 0;
                best = fminf(best, far ? FLT_MAX : d2);
                crossings += miss ? 0 : c;
                ++faces_tested;
            }
            const float r = sqrtf(best) + delta;
            bound = r * r * (1.f + 16.f * FLT_EPSILON);
        }
        if (seeding) { seeding = false; node = 1; continue; }
        node += 1;
        node >>= __ffs(node) - 1;
        if (node == 1) break;
    }
    sdist[i] = (crossings & 1) ? -sqrtf(best) : sqrtf(best);
    if (visits) { visits[2 * (size_t)i] = nodes_tested; visits[2 * (size_t)i + 1] = faces_tested; }
}

// Closest face: what k_mesh_closest (mesh_closest.hip) returns -- the lexicographic minimum of (d2, original face id) over the
// faces, d2 and q from tri_closest -- through the walk of k_index_sdist without its crossing column: a node is skipped when
// box_dist2 > bound and for no other reason.
// Slack.  tri_closest forms q = a + v ab + w ac and p - q with every product and sum rounded on its own (no fma): at most five
// roundings per component of q and one of p - q, each at most u M (u = 2^-24, M = the largest |coordinate| involved), so the
// value falls short of the true squared distance by what < 6 sqrt(3) u M < 11 u M in norm makes; barycentrics that rounding
// pushes out of [0, 1] move q along the face's plane by the same order.  That is the estimate of k_index_sdist's comment with
// two more roundings where tri_dist2 may have fused, and delta = 32 u M covers it three times over, so `bound` is formed as
// there: a face in a box with lb > bound returns d2 > best STRICTLY.  It can neither win nor tie, so the minimum of
// (d2, id) over the faces that are visited is the minimum over all faces, whatever the visiting order, and the answer has the
// bits of brute force.  A box at lb == bound is entered.  NaN (a zero-area face) and +inf fail both comparisons below.
// order: sorted slot -> original face id (the permutation given to mp_mesh_index_build), NULL = report sorted slots.
__global__ __launch_bounds__(QB) void k_index_closest(const float* __restrict__ pts, int n, const float* __restrict__ index, int F,
                                                      const long long* __restrict__ order, float* __restrict__ d2_out,
                                                      int* __restrict__ face_out, float* __restrict__ q_out,
                                                      int* __restrict__ visits) {
    const int i = blockIdx.x * QB + threadIdx.x;
    if (i >= n) return;
    const int NLp = n_leaves_pow2(F);
    const float4* nodes = reinterpret_cast<const float4*>(index + HDR_FLOATS);
    const float* faces = index + HDR_FLOATS + 16 * (size_t)NLp;
    const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    float best = INFINITY, bq[3] = {NAN, NAN, NAN};
    int bid = -1, nodes_tested = 0, faces_tested = 0;
    // a non-finite point has no closest face (fmaxf in box_dist2 would count a NaN axis as distance 0): no walk
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
        const float4 rlo = nodes[2], rhi = nodes[3];
        float M = fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]));
        M = fmaxf(M, fmaxf(fmaxf(fmaxf(fabsf(rlo.x), fabsf(rhi.x)), fmaxf(fabsf(rlo.y), fabsf(rhi.y))), fmaxf(fabsf(rlo.z), fabsf(rhi.z))));
        const float delta = 16.f * FLT_EPSILON * M;
        int seed = 1;
        while (seed < NLp) {
            const float dl = box_dist2(p, nodes[4 * seed], nodes[4 * seed + 1]), dr = box_dist2(p, nodes[4 * seed + 2], nodes[4 * seed + 3]);
            seed = dr < dl ? 2 * seed + 1 : 2 * seed;
            nodes_tested += 2;
        }
        float bound = INFINITY;            // nothing is far before the first face; stays +inf while best is (sqrtf(inf) = inf)
        bool seeding = true;
        int node = seed;
        for (int it = 0; it <= 2 * NLp; ++it) {
            ++nodes_tested;
            if (!(box_dist2(p, nodes[2 * node], nodes[2 * node + 1]) > bound)) {
                if (node < NLp) { node = 2 * node; continue; }
                const int l = node - NLp;
                for (int k = LEAF * l; k < min(LEAF * (l + 1), F); ++k) {
                    float a[9], q[3];
                    for (int e = 0; e < 9; ++e) a[e] = faces[9 * (size_t)k + e];
                    const float d2 = tri_closest(p, a, a + 3, a + 6, q);
                    const int id = order ? (int)order[k] : k;
                    if (d2 < best || (d2 == best && id < bid)) { best = d2; bid = id; bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2]; }
                    ++faces_tested;
                }
                const float r = sqrtf(best) + delta;
                bound = r * r * (1.f + 16.f * FLT_EPSILON);
            }
            if (seeding) { seeding = false; node = 1; continue; }
            node += 1;
            node >>= __ffs(node) - 1;
            if (node == 1) break;
        }
    }
    d2_out[i] = best;
    if (face_out) face_out[i] = bid;
    if (q_out) { q_out[3 * (size_t)i] = bq[0]; q_out[3 * (size_t)i + 1] = bq[1]; q_out[3 * (size_t)i + 2] = bq[2]; }
    if (visits) { visits[2 * (size_t)i] = nodes_tested; visits[2 * (size_t)i + 1] = faces_tested; }
}

}  // namespace

extern "C" int mp_mesh_index_bytes(int n_faces) {
    if (n_faces <= 0) return 0;
    return 4 * (HDR_FLOATS + 16 * n_leaves_pow2(n_faces) + 9 * LEAF * n_leaves(n_faces));
}

extern "C" int mp_mesh_index_keys(const float* face_verts, int n_faces, void* index, int* keys, void* stream) {
    if (n_faces <= 0) return -1;
    hipLaunchKernelGGL(k_index_bbox, dim3(1), dim3(1024), 0, (hipStream_t)stream, face_verts, n_faces, (float*)index);
    hipLaunchKernelGGL(k_index_keys, dim3((n_faces + 255) / 256), dim3(256), 0, (hipStream_t)stream, face_verts, n_faces,
                       (const float*)index, keys);
    return (int)hipGetLastError();
}

extern "C" int mp_mesh_index_build(const float* face_verts, int n_faces, const long long* order, void* index, void* stream) {
    if (n_faces <= 0) return -1;
    const int NLp = n_leaves_pow2(n_faces);
    float* nodes = (float*)index + HDR_FLOATS;
    float* faces = nodes + 16 * (size_t)NLp;
    hipLaunchKernelGGL(k_index_leaves, dim3((NLp + 255) / 256), dim3(256), 0, (hipStream_t)stream, face_verts, n_faces, order, nodes,
                       faces);
    int n = NLp / 2;
    for (; n > TOP; n >>= 1)
        hipLaunchKernelGGL(k_index_level, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, nodes, n);
    if (n >= 1) hipLaunchKernelGGL(k_index_top, dim3(1), dim3(TOP), 0, (hipStream_t)stream, nodes, n);
    return (int)hipGetLastError();
}

extern "C" int mp_mesh_index_signed_distance(const float* pts, int n, const void* index, int n_faces, float* sdist, int* visits,
                                             void* stream) {
    if (n <= 0) return 0;
    if (n_faces <= 0) return -1;
    hipLaunchKernelGGL(k_index_sdist, dim3((n + QB - 1) / QB), dim3(QB), 0, (hipStream_t)stream, pts, n, (const float*)index,
                       n_faces, sdist, visits);
    return (int)hipGetLastError();
}

extern "C" int mp_mesh_index_point_keys(const float* pts, int n, const void* index, int* keys, void* stream) {
    if (n < 0 || !index || (n > 0 && (!pts || !keys))) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_index_point_keys, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, n, (const float*)index,
                       keys);
    return (int)hipGetLastError();
}

extern "C" int mp_mesh_index_closest(const float* pts, int n, const void* index, int n_faces, const long long* order, float* d2,
                                     int* face, float* q, int* visits, void* stream) {
    if (n < 0 || n_faces <= 0 || !index || (n > 0 && (!pts || !d2))) return -1;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_index_closest, dim3((n + QB - 1) / QB), dim3(QB), 0, (hipStream_t)stream, pts, n, (const float*)index,
                       n_faces, order, d2, face, q, visits);
    return (int)hipGetLastError();
}
