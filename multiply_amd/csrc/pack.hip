// Weight packing: fp32 (optionally weight-normalised) nn.Linear parameters -> half (f16) MFMA A-fragments.
// Replaces nothing arithmetic in the reference except the weight-norm reparametrisation
// w = g * v / ||v|| (torch.nn.utils.weight_norm, reference networks.py:82-83) and hoists the per-call
// constant conditioning (networks.py:164-165) into the bias.  See include/multiply_hip.h: mp_pack_layer.
#include <hip/hip_runtime.h>
#include "../../include/multiply_hip.h"
#include "common.hpp"
#include "mlp_core.hpp"

namespace {

__global__ __launch_bounds__(64) void k_pack_layer(const float* __restrict__ v, const float* __restrict__ g,
                                                   const float* __restrict__ b, int out_dim, int in_dim,
                                                   const int* __restrict__ rowmap, const int* __restrict__ colmap,
                                                   const float* __restrict__ colscale, int ks_in, int hoist_col0,
                                                   int hoist_n, const float* __restrict__ hoist_vec, float bias_scale,
                                                   _Float16* __restrict__ wpack, float* __restrict__ bias_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int src = rowmap[r];
    const int n_slots = (mp::KS_REG + ks_in) * 32;
    const int mb = r >> 4, i = r & 15;
    float scale = 1.0f;
    const float* row = nullptr;
    if (src >= 0) {
        row = v + (size_t)src * in_dim;
        if (g) {
            float ss = 0.0f;
            for (int c = lane; c < in_dim; c += 64) ss += row[c] * row[c];
            ss = mp::wsum(ss);
            scale = g[src] / sqrtf(ss);
        }
    }
    if (wpack) {
        for (int s = lane; s < n_slots; s += 64) {
            float val = 0.0f;
            if (src >= 0) {
                const int col = colmap[s];
                if (col >= 0) val = row[col] * scale * colscale[s];
            }
            const int ks = s >> 5, sl = s & 31, gg = sl >> 3, e = sl & 7;
            const size_t off = ((size_t)(mb * (mp::KS_REG + ks_in) + ks) * 64 + (i + 16 * gg)) * 8 + e;
            wpack[off] = (_Float16)val;
        }
    }
    if (bias_out) {
        float h = 0.0f;
        if (src >= 0 && hoist_n > 0) {
            for (int c = lane; c < hoist_n; c += 64) h += (row[hoist_col0 + c] * scale) * hoist_vec[c];
            h = mp::wsum(h);
        }
        if (lane == 0) bias_out[r] = src >= 0 ? (b[src] + h) * bias_scale : 0.0f;
    }
}

// All layers of one network in ONE launch (mp_pack_layers): block (r, l) packs row r of layer l (or zeroes its bias entry).
__global__ __launch_bounds__(64) void k_pack_layers(const MpPackLayer* __restrict__ tab, int ks_in) {
    const MpPackLayer L = tab[blockIdx.y];
    const int r = blockIdx.x, lane = threadIdx.x;
    float* bias_out = (float*)L.bias_layer;
    if (r >= L.n_rows) {
        if (bias_out && lane == 0) bias_out[r] = 0.0f;
        return;
    }
    const float* v = (const float*)L.v;
    const float* g = (const float*)L.g;
    const float* b = (const float*)L.b;
    const int* rowmap = (const int*)L.rowmap;
    const int* colmap = (const int*)L.colmap;
    const float* colscale = (const float*)L.colscale;
    const float* hoist_vec = (const float*)L.hoist_vec;
    _Float16* wpack = (_Float16*)L.wpack_layer;
    const int src = rowmap[r];
    const int n_slots = (mp::KS_REG + ks_in) * 32;
    const int mb = r >> 4, i = r & 15;
    float scale = 1.0f;
    const float* row = nullptr;
    if (src >= 0) {
        row = v + (size_t)src * L.in_dim;
        if (g) {
            float ss = 0.0f;
            for (int c = lane; c < L.in_dim; c += 64) ss += row[c] * row[c];
            ss = mp::wsum(ss);
            scale = g[src] / sqrtf(ss);
        }
    }
    if (wpack) {
        for (int s = lane; s < n_slots; s += 64) {
            float val = 0.0f;
            if (src >= 0) {
                const int col = colmap[s];
                if (col >= 0) val = row[col] * scale * colscale[s];
            }
            const int ks = s >> 5, sl = s & 31, gg = sl >> 3, e = sl & 7;
            const size_t off = ((size_t)(mb * (mp::KS_REG + ks_in) + ks) * 64 + (i + 16 * gg)) * 8 + e;
            wpack[off] = (_Float16)val;
        }
    }
    if (bias_out) {
        float h = 0.0f;
        if (src >= 0 && L.hoist_n > 0 && hoist_vec) {
            for (int c = lane; c < L.hoist_n; c += 64) h += (row[L.hoist_col0 + c] * scale) * hoist_vec[c];
            h = mp::wsum(h);
        }
        if (lane == 0) bias_out[r] = src >= 0 ? (b[src] + h) * L.bias_scale : 0.0f;
    }
}

// Feature fold (mp_fold_features): block r builds row r of the colour network's first layer with the SDF network's last layer
// multiplied in.  256 threads; cold path (runs when a parameter of either layer changed).
constexpr int FOLD_MAX_FEAT = 1024;
__global__ __launch_bounds__(256) void k_fold_features(const float* __restrict__ vc, const float* __restrict__ gc,
                                                       const float* __restrict__ bc, int in_c, int feat_col0, int n_feat,
                                                       const float* __restrict__ v8, const float* __restrict__ g8,
                                                       const float* __restrict__ b8, int in8, float* __restrict__ out_w,
                                                       float* __restrict__ out_b) {
    __shared__ float a[FOLD_MAX_FEAT];   // Wc_eff[r][feat_col0 + f] * (weight-norm factor of row 1 + f of the SDF layer)
    __shared__ float sh[4];
    const int r = blockIdx.x, t = threadIdx.x;
    const float* row = vc + (size_t)r * in_c;
    float sc = 1.0f;
    if (gc) {
        float ss = 0.0f;
        for (int c = t; c < in_c; c += 256) ss += row[c] * row[c];
        sc = gc[r] / sqrtf(mp::block_sum256(ss, sh));
    }
    float bsum = 0.0f;
    for (int f = t; f < n_feat; f += 256) {
        const float w = row[feat_col0 + f] * sc;
        float s8 = 1.0f;
        if (g8) {
            const float* r8 = v8 + (size_t)(1 + f) * in8;
            float ss = 0.0f;
            for (int k = 0; k < in8; ++k) ss += r8[k] * r8[k];
            s8 = g8[1 + f] / sqrtf(ss);
        }
        a[f] = w * s8;
        bsum += w * b8[1 + f];
    }
    bsum = mp::block_sum256(bsum, sh);   // (its barriers also publish a[])
    float* orow = out_w + (size_t)r * in_c;
    for (int c = t; c < in_c; c += 256)
        if (c < feat_col0 || c >= feat_col0 + n_feat) orow[c] = row[c] * sc;
    for (int k = t; k < n_feat; k += 256) {
        float acc = 0.0f;
        if (k < in8)
            for (int f = 0; f < n_feat; ++f) acc = __builtin_fmaf(a[f], v8[(size_t)(1 + f) * in8 + k], acc);
        orow[feat_col0 + k] = acc;
    }
    if (t == 0) out_b[r] = bc[r] + bsum;
}

__global__ void k_zero_f(float* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}

}  // namespace

extern "C" int mp_pack_layer(const float* v, const float* g, const float* b, int out_dim, int in_dim,
                             const int* rowmap, int n_rows, const int* colmap, const float* colscale, int ks_in,
                             int hoist_col0, int hoist_n, const float* hoist_vec, float bias_scale,
                             void* wpack_layer, float* bias_layer, void* stream) {
    if (n_rows <= 0 || n_rows % 32 || n_rows > MP_BIAS_STRIDE || (ks_in != 0 && ks_in != 2 && ks_in != 3)) return -1;
    hipStream_t st = (hipStream_t)stream;
    if (bias_layer && n_rows < MP_BIAS_STRIDE)
        hipLaunchKernelGGL(k_zero_f, dim3(1), dim3(MP_BIAS_STRIDE), 0, st, bias_layer + n_rows, MP_BIAS_STRIDE - n_rows);
    hipLaunchKernelGGL(k_pack_layer, dim3(n_rows), dim3(64), 0, st, v, g, b, out_dim, in_dim, rowmap, colmap,
                       colscale, ks_in, hoist_col0, hoist_n, hoist_vec, bias_scale, (_Float16*)wpack_layer, bias_layer);
    return (int)hipGetLastError();
}

extern "C" int mp_pack_layers(const MpPackLayer* table, int n_layers, int ks_in, void* stream) {
    if (n_layers <= 0 || n_layers > MP_MAX_LAYERS || (ks_in != 0 && ks_in != 2 && ks_in != 3)) return -1;
    hipLaunchKernelGGL(k_pack_layers, dim3(MP_BIAS_STRIDE, n_layers), dim3(64), 0, (hipStream_t)stream, table, ks_in);
    return (int)hipGetLastError();
}

extern "C" int mp_fold_features(const float* vc, const float* gc, const float* bc, int out_c, int in_c, int feat_col0,
                                int n_feat, const float* v8, const float* g8, const float* b8, int in8, float* out_w,
                                float* out_b, void* stream) {
    if (out_c <= 0 || n_feat <= 0 || n_feat > FOLD_MAX_FEAT || feat_col0 < 0 || feat_col0 + n_feat > in_c || in8 <= 0 ||
        in8 > n_feat)
        return -1;
    hipLaunchKernelGGL(k_fold_features, dim3(out_c), dim3(256), 0, (hipStream_t)stream, vc, gc, bc, in_c, feat_col0, n_feat,
                       v8, g8, b8, in8, out_w, out_b);
    return (int)hipGetLastError();
}

extern "C" const char* mp_arch(void) { return "gfx950"; }

extern "C" int mp_device_ok(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    const char* a = prop.gcnArchName;
    return (a[0] == 'g' && a[1] == 'f' && a[2] == 'x' && a[3] == '9' && a[4] == '5' && a[5] == '0') ? 1 : 0;
}
