// Projection, pixel box and coverage of the hard rasterisation rule (the header comment of raster.hip), shared by raster.hip
// (mp_raster_zbuf, mp_raster_mask_batch) and overlay.hip (mp_overlay_batch) so that all three decide a pixel with the same
// arithmetic.  Moved here from raster.hip textually unchanged.  The CALLERS' loop shapes matter too: see k_mask_big's note.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int SMALL_BOX = 48;   // pixel tests a single thread does before the face goes to the workgroup queue
constexpr float K_EPS = 1e-8f;

struct Cam {
    float R[9], T[3], fx, fy, cx, cy, z_clip;
};

struct Tri {
    float x0, y0, z0, x1, y1, z1, x2, y2, z2, area;
};

__device__ __forceinline__ void project(const Cam& c, const float* __restrict__ v, float& x, float& y, float& z) {
    const float X = c.R[0] * v[0] + c.R[1] * v[1] + c.R[2] * v[2] + c.T[0];
    const float Y = c.R[3] * v[0] + c.R[4] * v[1] + c.R[5] * v[2] + c.T[1];
    z = c.R[6] * v[0] + c.R[7] * v[1] + c.R[8] * v[2] + c.T[2];
    x = c.fx * X / z + c.cx;
    y = c.fy * Y / z + c.cy;
}

// edge(p; a, b) of pytorch3d's EdgeFunctionForward
__device__ __forceinline__ float edge(float px, float py, float ax, float ay, float bx, float by) {
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

__device__ __forceinline__ bool load_tri(const Cam& c, const float* __restrict__ verts, const int* __restrict__ faces, int f,
                                         Tri& t) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    project(c, verts + 3 * (size_t)i0, t.x0, t.y0, t.z0);
    project(c, verts + 3 * (size_t)i1, t.x1, t.y1, t.z1);
    project(c, verts + 3 * (size_t)i2, t.x2, t.y2, t.z2);
    if (!(fminf(t.z0, fminf(t.z1, t.z2)) >= c.z_clip)) return false;   // dropped, not clipped (see the header)
    t.area = edge(t.x2, t.y2, t.x0, t.y0, t.x1, t.y1);
    return fabsf(t.area) > K_EPS;
}

// perspective-correct barycentrics and depth of pixel centre (px, py); false = not covered
__device__ __forceinline__ bool cover(const Tri& t, float px, float py, float& b0, float& b1, float& b2, float& pz) {
    const float a = t.area + K_EPS;
    const float w0 = edge(px, py, t.x1, t.y1, t.x2, t.y2) / a;
    const float w1 = edge(px, py, t.x2, t.y2, t.x0, t.y0) / a;
    const float w2 = edge(px, py, t.x0, t.y0, t.x1, t.y1) / a;
    if (!(w0 > 0.f && w1 > 0.f && w2 > 0.f)) return false;
    const float t0 = w0 * t.z1 * t.z2, t1 = t.z0 * w1 * t.z2, t2 = t.z0 * t.z1 * w2;
    const float d = fmaxf(t0 + t1 + t2, K_EPS);
    b0 = t0 / d; b1 = t1 / d; b2 = t2 / d;
    pz = b0 * t.z0 + b1 * t.z1 + b2 * t.z2;
    return pz >= 0.f;
}

__device__ __forceinline__ bool pixel_box(const Tri& t, int H, int W, int& c0, int& c1, int& r0, int& r1) {
    const float xmin = fminf(t.x0, fminf(t.x1, t.x2)), xmax = fmaxf(t.x0, fmaxf(t.x1, t.x2));
    const float ymin = fminf(t.y0, fminf(t.y1, t.y2)), ymax = fmaxf(t.y0, fmaxf(t.y1, t.y2));
    if (!(xmax >= 0.f && ymax >= 0.f && xmin <= (float)W && ymin <= (float)H)) return false;   // also rejects NaN
    c0 = max(0, (int)ceilf(xmin - 0.5f));      // pixel centres c + 0.5 inside [xmin, xmax]
    c1 = min(W - 1, (int)floorf(xmax - 0.5f));
    r0 = max(0, (int)ceilf(ymin - 0.5f));
    r1 = min(H - 1, (int)floorf(ymax - 0.5f));
    return c0 <= c1 && r0 <= r1;
}

}  // namespace
