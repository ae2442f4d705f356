// Point-triangle primitives of the mesh signed distance, shared by the brute-force kernel (mesh.hip, k_mesh_sdist) and the
// indexed one (mesh_index.hip, k_index_sdist): both must evaluate a face with the SAME arithmetic, since the indexed kernel is
// defined as "what brute force returns, without visiting the faces that cannot matter".
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// squared distance from p to triangle (a, b, c)
__device__ __forceinline__ float tri_dist2(const float* p, const float* a, const float* b, const float* c) {
    float ab[3], ac[3], ap[3];
    for (int i = 0; i < 3; ++i) { ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; ap[i] = p[i] - a[i]; }
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    float q[3];
    if (d1 <= 0.f && d2 <= 0.f) { for (int i = 0; i < 3; ++i) q[i] = a[i]; }
    else {
        float bp[3];
        for (int i = 0; i < 3; ++i) bp[i] = p[i] - b[i];
        const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
        if (d3 >= 0.f && d4 <= d3) { for (int i = 0; i < 3; ++i) q[i] = b[i]; }
        else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
                const float v = d1 / (d1 - d3);
                for (int i = 0; i < 3; ++i) q[i] = a[i] + v * ab[i];
            } else {
                float cp[3];
                for (int i = 0; i < 3; ++i) cp[i] = p[i] - c[i];
                const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
                if (d6 >= 0.f && d5 <= d6) { for (int i = 0; i < 3; ++i) q[i] = c[i]; }
                else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
                        const float w = d2 / (d2 - d6);
                        for (int i = 0; i < 3; ++i) q[i] = a[i] + w * ac[i];
                    } else {
                        const float va = d3 * d6 - d5 * d4;
                        if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
                            const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                            for (int i = 0; i < 3; ++i) q[i] = b[i] + w * (c[i] - b[i]);
                        } else {
                            const float den = 1.0f / (va + vb + vc);
                            const float v = vb * den, w = vc * den;
                            for (int i = 0; i < 3; ++i) q[i] = a[i] + ab[i] * v + ac[i] * w;
                        }
                    }
                }
            }
        }
    }
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return dx * dx + dy * dy + dz * dz;
}

// Closest point q of triangle (a, b, c) to p and the squared distance |p - q|^2: the region classification of tri_dist2 (Ericson,
// Real-Time Collision Detection 5.1.5), shared by the brute-force and the indexed closest-face kernels (mesh_closest.hip,
// mesh_index.hip), which must agree bit for bit.  Unlike tri_dist2 the value does not depend on where the function is inlined:
// contraction is off in every statement (each product and sum is rounded on its own, no fma is formed from them), the divides
// are correctly rounded, and nothing here is reassociated -- d2 and q are a function of (p, a, b, c) alone.  That is why the
// dot products are spelled out below instead of calling dot3, whose operations carry the file's default contraction.
// A face of zero area -- (b - a) x (c - a) == 0 exactly, e.g. a repeated vertex -- has no closest point: q = NaN, d2 = NaN,
// which no selection takes.  (tri_dist2 answers such a face with NaN or with the distance to a vertex, whichever region p hits.)
__device__ __forceinline__ float tri_closest(const float* p, const float* a, const float* b, const float* c, float* q) {
#pragma clang fp contract(off)
    float ab[3], ac[3], ap[3];
    for (int i = 0; i < 3; ++i) { ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; ap[i] = p[i] - a[i]; }
    const float nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    if (nx == 0.f && ny == 0.f && nz == 0.f) {
        q[0] = q[1] = q[2] = __builtin_nanf("");
        return __builtin_nanf("");
    }
    const float d1 = (ab[0] * ap[0] + ab[1] * ap[1]) + ab[2] * ap[2], d2 = (ac[0] * ap[0] + ac[1] * ap[1]) + ac[2] * ap[2];
    if (d1 <= 0.f && d2 <= 0.f) { for (int i = 0; i < 3; ++i) q[i] = a[i]; }
    else {
        float bp[3];
        for (int i = 0; i < 3; ++i) bp[i] = p[i] - b[i];
        const float d3 = (ab[0] * bp[0] + ab[1] * bp[1]) + ab[2] * bp[2], d4 = (ac[0] * bp[0] + ac[1] * bp[1]) + ac[2] * bp[2];
        if (d3 >= 0.f && d4 <= d3) { for (int i = 0; i < 3; ++i) q[i] = b[i]; }
        else {
            const float vc = d1 * d4 - d3 * d2;
            if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
                const float v = d1 / (d1 - d3);
                for (int i = 0; i < 3; ++i) q[i] = a[i] + v * ab[i];
            } else {
                float cp[3];
                for (int i = 0; i < 3; ++i) cp[i] = p[i] - c[i];
                const float d5 = (ab[0] * cp[0] + ab[1] * cp[1]) + ab[2] * cp[2], d6 = (ac[0] * cp[0] + ac[1] * cp[1]) + ac[2] * cp[2];
                if (d6 >= 0.f && d5 <= d6) { for (int i = 0; i < 3; ++i) q[i] = c[i]; }
                else {
                    const float vb = d5 * d2 - d1 * d6;
                    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
                        const float w = d2 / (d2 - d6);
                        for (int i = 0; i < 3; ++i) q[i] = a[i] + w * ac[i];
                    } else {
                        const float va = d3 * d6 - d5 * d4;
                        if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
                            const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
                            for (int i = 0; i < 3; ++i) q[i] = b[i] + w * (c[i] - b[i]);
                        } else {
                            const float den = 1.0f / ((va + vb) + vc);
                            const float v = vb * den, w = vc * den;
                            for (int i = 0; i < 3; ++i) q[i] = (a[i] + ab[i] * v) + ac[i] * w;
                        }
                    }
                }
            }
        }
    }
    const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// does the ray p + t (1,0,0), t > 0 cross the triangle?  (y,z) projection, half-open edges: an edge (u,v) counts when
// exactly one endpoint has y > p.y; the crossing is inside when the edge functions agree in sign.
__device__ __forceinline__ bool ray_x_crosses(const float* p, const float* a, const float* b, const float* c) {
    // 2D point-in-triangle in (y,z) by the crossing-number rule along +z, then the x of the plane point
    int cn = 0;
    const float* v[3] = {a, b, c};
    for (int e = 0; e < 3; ++e) {
        const float* u = v[e];
        const float* w = v[(e + 1) % 3];
        const bool uy = u[1] > p[1], wy = w[1] > p[1];
        if (uy != wy) {
            const float t = (p[1] - u[1]) / (w[1] - u[1]);
            const float zc = u[2] + t * (w[2] - u[2]);
            if (zc > p[2]) ++cn;
        }
    }
    if ((cn & 1) == 0) return false;
    // plane: n . (x - a) = 0 -> x at (p.y, p.z)
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    if (nx == 0.f) return false;   // triangle parallel to the ray
    const float x = a[0] - (ny * (p[1] - a[1]) + nz * (p[2] - a[2])) / nx;
    return x > p[0];
}

}  // namespace
