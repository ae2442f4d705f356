// Shaded mesh overlays for a batch of meshes: the QC images the reference writes at every preprocessing stage
// (preprocessing/preprocessing_multiple_trace.py:330-342, 496-510: init_smpl_image/, init_refined_smpl/) and for the
// reconstructed meshes (ait_viewer_vis/vis_mesh_image.py).  The reference draws them one mesh at a time through pytorch3d (hard
// rasteriser, 10-face depth softmax) and cv2.circle; both are third party and unpinned, so the rule here is the project's own:
//   * visibility is mp_raster_zbuf's (raster.hip's header comment): pixel centres, cover(), faces dropped at z_clip, the
//     nearest depth wins -- the same projection, box and coverage functions (raster_prims.hpp), called from loops of the same
//     shape as raster.hip's (k_mask_big's note: another loop shape contracts other multiply-adds and outline pixels flip);
//   * the winner's colour is the perspective-correct barycentric mean of its three vertex colours, cut to a byte with floor,
//     blended over the frame byte f as floor(fmaf(opacity, m - f, f) + 0.5);
//   * a keypoint is the integer disc (c - floor x)^2 + (r - floor y)^2 <= radius^2, painted last, the highest index on top.
//
// Layout for MI355X: as raster.hip's z-buffer, scattered rather than tiled (~1 pixel per face at image scale) -- one thread per
// face walks the face's pixel box, one 64-bit atomicMin per covered pixel; large boxes go to a queue that a second launch sweeps
// with a workgroup per face.  What is new is the batch: the meshes come as a DEVICE table of records (as mp_adam_multi's tensor
// table), the grid is the records' face blocks concatenated and a block finds its record by binary search (as k_wn_fwd_multi),
// so a 300-frame sequence is five launches and no host read.  The key's low word is the GLOBAL face id face_base[record] + f:
// ties go to the earlier record, then the lower face, independent of scheduling, and the resolve pass finds the record back by
// binary search in face_base.  Cameras are per image, so they live in device memory (16 floats each, copied from the host
// array by the entry point) and every thread builds its Cam from there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "raster_prims.hpp"

namespace {

constexpr unsigned long long EMPTY_KEY = ~0ull;

__device__ __forceinline__ Cam load_cam(const float* __restrict__ cams, int n_cam, int image, float z_clip) {
    const float* c = cams + 16 * (size_t)(n_cam == 1 ? 0 : image);
    Cam cam;
    for (int i = 0; i < 9; ++i) cam.R[i] = c[i];
    for (int i = 0; i < 3; ++i) cam.T[i] = c[9 + i];
    cam.fx = c[12]; cam.fy = c[13]; cam.cx = c[14]; cam.cy = c[15];
    cam.z_clip = z_clip;
    return cam;
}

// last record whose block0 <= b: records without faces have no block and share their block0 with the record that follows
__device__ __forceinline__ int record_of_block(const MpOverlayMesh* __restrict__ recs, int n_rec, int b) {
    int lo = 0, hi = n_rec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// last record whose face_base <= g (the same remark)
__device__ __forceinline__ int record_of_face(const MpOverlayMesh* __restrict__ recs, int n_rec, unsigned g) {
    int lo = 0, hi = n_rec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].face_base <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void splat(const Tri& t, unsigned g, int r, int c, int W, unsigned long long* __restrict__ keys) {
    float b0, b1, b2, pz;
    if (cover(t, c + 0.5f, r + 0.5f, b0, b1, b2, pz))
        atomicMin(keys + (size_t)r * W + c, ((unsigned long long)__float_as_uint(pz) << 32) | g);
}

__global__ __launch_bounds__(256) void k_overlay_faces(const MpOverlayMesh* __restrict__ recs, int n_rec,
                                                       const float* __restrict__ cams, int n_cam, float z_clip, int M, int H,
                                                       int W, unsigned long long* __restrict__ keys, unsigned* __restrict__ big) {
    const int ri = record_of_block(recs, n_rec, (int)blockIdx.x);
    const MpOverlayMesh rec = recs[ri];
    const int f = ((int)blockIdx.x - rec.block0) * 256 + (int)threadIdx.x;
    if (f >= rec.n_faces || (unsigned)rec.image >= (unsigned)M) return;      // a record outside the images draws nothing
    const Cam cam = load_cam(cams, n_cam, rec.image, z_clip);
    Tri t;
    int c0, c1, r0, r1;
    if (!load_tri(cam, rec.verts, rec.faces, f, t) || !pixel_box(t, H, W, c0, c1, r0, r1)) return;
    const unsigned g = rec.face_base + (unsigned)f;
    if ((c1 - c0 + 1) * (long long)(r1 - r0 + 1) > SMALL_BOX) {
        big[1 + atomicAdd(big, 1u)] = g;
        return;
    }
    unsigned long long* k = keys + (size_t)rec.image * H * W;
    for (int r = r0; r <= r1; ++r)
        for (int c = c0; c <= c1; ++c) splat(t, g, r, c, W, k);
}

// one workgroup per queued face; the queue length lives on the device
__global__ __launch_bounds__(256) void k_overlay_big(const MpOverlayMesh* __restrict__ recs, int n_rec,
                                                     const float* __restrict__ cams, int n_cam, float z_clip, int H, int W,
                                                     unsigned long long* __restrict__ keys, const unsigned* __restrict__ big) {
    const unsigned n = big[0];
    for (unsigned q = blockIdx.x; q < n; q += gridDim.x) {
        const unsigned g = big[1 + q];
        const MpOverlayMesh rec = recs[record_of_face(recs, n_rec, g)];
        const int f = (int)(g - rec.face_base);
        const Cam cam = load_cam(cams, n_cam, rec.image, z_clip);
        Tri t;
        int c0, c1, r0, r1;
        if (!load_tri(cam, rec.verts, rec.faces, f, t) || !pixel_box(t, H, W, c0, c1, r0, r1)) continue;
        unsigned long long* k = keys + (size_t)rec.image * H * W;
        const int bw = c1 - c0 + 1;
        const long long np = (long long)bw * (r1 - r0 + 1);
        for (long long i = threadIdx.x; i < np; i += blockDim.x) splat(t, g, r0 + (int)(i / bw), c0 + (int)(i % bw), W, k);
    }
}

struct OverlayPaint {
    float opacity, kp_conf;
    int K, kp_radius;
    unsigned char bg[3];
};

__global__ __launch_bounds__(256) void k_overlay_resolve(const MpOverlayMesh* __restrict__ recs, int n_rec,
                                                         const float* __restrict__ cams, int n_cam, float z_clip, int M, int H,
                                                         int W, const unsigned long long* __restrict__ keys,
                                                         const unsigned char* __restrict__ frames,
                                                         const float* __restrict__ keypoints,
                                                         const unsigned char* __restrict__ kp_rgb, OverlayPaint pp,
                                                         unsigned char* __restrict__ out, int* __restrict__ owner) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x, npix = (size_t)H * W;
    if (p >= (size_t)M * npix) return;
    const int image = (int)(p / npix);
    const int q = (int)(p - (size_t)image * npix), r = q / W, c = q % W;
    float fr[3];
    for (int ch = 0; ch < 3; ++ch) fr[ch] = frames ? (float)frames[3 * p + ch] : (float)pp.bg[ch];
    unsigned char o[3] = {(unsigned char)fr[0], (unsigned char)fr[1], (unsigned char)fr[2]};
    int who = -1;
    const unsigned long long k = keys[p];
    if (k != EMPTY_KEY) {
        const unsigned g = (unsigned)(k & 0xffffffffull);
        who = record_of_face(recs, n_rec, g);
        const MpOverlayMesh rec = recs[who];
        const int f = (int)(g - rec.face_base);
        const Cam cam = load_cam(cams, n_cam, image, z_clip);
        Tri t;
        load_tri(cam, rec.verts, rec.faces, f, t);
        float b0 = 0.f, b1 = 0.f, b2 = 0.f, pz;
        cover(t, (float)c + 0.5f, (float)r + 0.5f, b0, b1, b2, pz);
        const float* c0 = rec.colors + 3 * (size_t)rec.faces[3 * f];
        const float* c1 = rec.colors + 3 * (size_t)rec.faces[3 * f + 1];
        const float* c2 = rec.colors + 3 * (size_t)rec.faces[3 * f + 2];
        for (int ch = 0; ch < 3; ++ch) {
            const float col = fmaf(b2, c2[ch], fmaf(b1, c1[ch], b0 * c0[ch]));
            const float m = floorf(255.f * fminf(fmaxf(col, 0.f), 1.f));        // fmaxf / fminf: a NaN colour gives 0
            o[ch] = (unsigned char)floorf(fmaf(pp.opacity, m - fr[ch], fr[ch]) + 0.5f);
        }
    }
    int kp = -1;
    for (int j = 0; j < pp.K; ++j) {
        const float* kj = keypoints + 3 * ((size_t)image * pp.K + j);
        const float x = kj[0], y = kj[1];
        if (!(kj[2] > pp.kp_conf) || !isfinite(x) || !isfinite(y)) continue;
        // |offset| <= radius first, in floats (exact below 2^24, and beyond it no pixel is that near): then the ints are small
        const float dxf = (float)c - floorf(x), dyf = (float)r - floorf(y);
        if (!(fabsf(dxf) <= (float)pp.kp_radius && fabsf(dyf) <= (float)pp.kp_radius)) continue;
        const int dx = (int)dxf, dy = (int)dyf;
        if (dx * dx + dy * dy <= pp.kp_radius * pp.kp_radius) kp = j;
    }
    if (kp >= 0)
        for (int ch = 0; ch < 3; ++ch) o[ch] = kp_rgb[3 * kp + ch];
    for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = o[ch];
    if (owner) owner[p] = who;
}

// ---------------------------------------------------------------------------------------------------------------------
// Vertex normals (render.py's render_mesh_recon: the area-weighted sum of the adjacent face normals, normalised with eps 1e-6)
// as a gather over a vertex -> face CSR: faces ascending, no atomics, so the sum's order -- and with it every bit -- is fixed.
__global__ __launch_bounds__(256) void k_vertex_normals(const float* __restrict__ verts, long long total, int V,
                                                        const int* __restrict__ faces, const int* __restrict__ adj_ptr,
                                                        const int* __restrict__ adj_face, float* __restrict__ normals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int v = (int)(i % V);
    const float* mv = verts + (size_t)(i / V) * V * 3;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int a = adj_ptr[v]; a < adj_ptr[v + 1]; ++a) {
        const int f = adj_face[a];
        const float* p0 = mv + 3 * (size_t)faces[3 * f];
        const float* p1 = mv + 3 * (size_t)faces[3 * f + 1];
        const float* p2 = mv + 3 * (size_t)faces[3 * f + 2];
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        sx += ay * bz - az * by;
        sy += az * bx - ax * bz;
        sz += ax * by - ay * bx;
    }
    const float len = fmaxf(sqrtf(sx * sx + sy * sy + sz * sz), 1e-6f);
    normals[3 * i] = sx / len;
    normals[3 * i + 1] = sy / len;
    normals[3 * i + 2] = sz / len;
}

__global__ __launch_bounds__(256) void k_vertex_colors(const float* __restrict__ normals, long long total, int V, int mode,
                                                       const float* __restrict__ tint, float lx, float ly, float lz, float ambient,
                                                       float* __restrict__ colors) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    float r, g, b;
    if (mode == MP_OVERLAY_NORMAL) {
        r = nz * 0.5f + 0.5f; g = ny * 0.5f + 0.5f; b = nx * 0.5f + 0.5f;
    } else {
        const float d = fmaxf(nx * lx + ny * ly + nz * lz, 0.f);
        if (mode == MP_OVERLAY_SHADE) {
            r = g = b = d;
        } else {
            const float s = ambient + (1.f - ambient) * d;
            const float* t = tint + 3 * (size_t)(i / V);
            r = t[0] * s; g = t[1] * s; b = t[2] * s;
        }
    }
    colors[3 * i] = r; colors[3 * i + 1] = g; colors[3 * i + 2] = b;
}

}  // namespace

extern "C" int mp_mesh_vertex_normals(const float* verts, int N, int V, const int* faces, int n_faces, const int* adj_ptr,
                                      const int* adj_face, float* normals, void* stream) {
    if (N < 0 || V < 0 || n_faces < 0) return -1;
    const long long total = (long long)N * V;
    if (total == 0) return 0;
    if (!verts || !adj_ptr || !normals || (n_faces > 0 && (!faces || !adj_face)) || total > 0x7fffffffLL - 1) return -1;
    hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, total, V,
                       faces, adj_ptr, adj_face, normals);
    return (int)hipGetLastError();
}

extern "C" int mp_overlay_vertex_colors(const float* normals, int N, int V, int mode, const float* tint, float lx, float ly,
                                        float lz, float ambient, float* colors, void* stream) {
    if (N < 0 || V < 0) return -1;
    if (mode != MP_OVERLAY_NORMAL && mode != MP_OVERLAY_SHADE && mode != MP_OVERLAY_TINT) return -2;
    const long long total = (long long)N * V;
    if (total == 0) return 0;
    if (!normals || !colors || (mode == MP_OVERLAY_TINT && !tint) || total > 0x7fffffffLL - 1) return -1;
    hipLaunchKernelGGL(k_vertex_colors, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, normals, total, V,
                       mode, tint, lx, ly, lz, ambient, colors);
    return (int)hipGetLastError();
}

extern "C" int mp_overlay_batch(const MpOverlayMesh* recs, int n_rec, int total_blocks, long long total_faces, int M, int H, int W,
                                const float* cams_host, int n_cam, float z_clip, const unsigned char* frames,
                                const unsigned char* background_host, float opacity, const float* keypoints, int K,
                                const unsigned char* kp_rgb, float kp_conf, int kp_radius, unsigned long long* keys, unsigned* big,
                                float* cam_dev, unsigned char* out, int* owner, void* stream) {
    if (n_rec < 0 || total_blocks < 0 || total_faces < 0 || M < 0 || K < 0 || H <= 0 || W <= 0) return -1;
    if (M == 0) return 0;
    if (!cams_host || !keys || !cam_dev || !out || (!frames && !background_host)) return -1;
    if (n_rec > 0 && (!recs || !big)) return -1;
    if (K > 0 && (!keypoints || !kp_rgb)) return -1;
    const long long npix = (long long)M * H * W;
    if (npix > 0x7fffffffLL - 1) return -1;
    if (n_cam != 1 && n_cam != M) return -2;
    if (total_faces >= 0xffffffffLL) return -2;                       // the key's low word; 2^32 - 1 marks an empty pixel
    if (!(opacity >= 0.f && opacity <= 1.f) || kp_radius < 0 || kp_radius > 4096) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)npix * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyAsync(cam_dev, cams_host, (size_t)n_cam * 16 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return (int)e;
    if (n_rec > 0 && total_blocks > 0) {
        e = hipMemsetAsync(big, 0, sizeof(unsigned), st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_overlay_faces, dim3((unsigned)total_blocks), dim3(256), 0, st, recs, n_rec, cam_dev, n_cam, z_clip, M, H,
                           W, keys, big);
        hipLaunchKernelGGL(k_overlay_big, dim3((unsigned)(total_faces < 2048 ? (total_faces > 0 ? total_faces : 1) : 2048)),
                           dim3(256), 0, st, recs, n_rec, cam_dev, n_cam, z_clip, H, W, keys, big);
    }
    OverlayPaint pp;
    pp.opacity = opacity; pp.kp_conf = kp_conf; pp.K = K; pp.kp_radius = kp_radius;
    for (int i = 0; i < 3; ++i) pp.bg[i] = frames ? 0 : background_host[i];
    hipLaunchKernelGGL(k_overlay_resolve, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, recs, n_rec, cam_dev, n_cam,
                       z_clip, M, H, W, keys, frames, keypoints, kp_rgb, pp, out, owner);
    return (int)hipGetLastError();
}
