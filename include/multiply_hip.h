/* multiply_hip.h — C ABI of libmultiply_hip.so (gfx950 / MI355X).
 *
 * The reference (eth-ait/MultiPly) has no FFI: its hot path is PyTorch code under
 * code/lib/model/ that is entered through Multiply.forward (code/lib/model/multiply.py:174).
 * This library is the boundary introduced BELOW that Python signature: every entry point
 * takes raw device pointers, sizes and a hipStream_t (as void*), allocates nothing, never
 * throws, and returns 0 on success or a hipError_t / negative argument-error code.
 * multiply_amd/hip.py is the ctypes binding a maintainer would add to the reference
 * (see INTEGRATION.md); each entry point names the reference code it replaces.
 *
 * All float tensors are fp32, row-major, contiguous.  "count pointers" are device ints so that
 * data-dependent sizes never need a host round trip: kernels are launched for the upper bound
 * and read the real count on the device.
 */
#ifndef MULTIPLY_HIP_H
#define MULTIPLY_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MP_MAX_LAYERS 10
#define MP_MAX_CHUNKS 9
#define MP_BIAS_STRIDE 288 /* floats per layer in a packed bias table */
#define MP_SMPL_V 6890
#define MP_SMPL_J 24
#ifndef MP_KNN_CLUSTER      /* (overridable for experiments: -DMP_KNN_CLUSTER=32 -DMP_KNN_NC=216 + the same two environment variables for hip.py) */
#define MP_KNN_CLUSTER 32   /* vertices per nearest-neighbour cluster (a power of two <= 64).  Round 6: 32 x 216 instead of 64 x 108 -- the */
#define MP_KNN_NC 216       /* clusters (216*32 = 6912 >= 6890, padded); <= 511.  cluster scan is wave-uniform, so finer clusters prune   */
                            /* better: sampler warp -19 %, Jacobian -18 %, frame -1.4 ms; 16 x 431: another -0.4 ms, training +0.8 ms    */
#endif

enum { MP_ACT_NONE = 0, MP_ACT_SOFTPLUS = 1, MP_ACT_RELU = 2, MP_ACT_SIGMUL = 3 };

typedef struct {
    int n_chunk;   /* chunks of 32 output rows */
    int use_reg;   /* layer consumes the 256 register-fed K slots (previous layer output) */
    int use_in;    /* layer consumes the 64/96 input-fed K slots (encoded network input) */
    int act;       /* MP_ACT_* */
    int out_chunk; /* chunk returned in fp32 instead of feeding the next layer, -1 = none */
    int aux;       /* reverse sweep only (MP_ACT_SIGMUL): bits 0..7 = 1 + stored-sigmoid layer, bits 8..15 = capture id */
} MpLayer;

typedef struct {
    int n_layers;
    int total_chunks;
    MpLayer layer[MP_MAX_LAYERS];
} MpNet;

/* ---- weights -------------------------------------------------------------------------------
 * Packs one linear layer (optionally weight-normalised: w = g * v / ||v||_row,
 * networks.py:82-83) into the half (f16) MFMA-fragment layout of csrc/mlp_core.hpp and writes its
 * fp32 bias row, with an optional hoisted contribution  bias[r] += sum_c W[r][hoist_col0+c] *
 * hoist_vec[c]  (the pose / frame conditioning that the reference concatenates to every point,
 * networks.py:164-165, 279-281, 275-276, is the same for all points of a call).
 *   v [out_dim][in_dim], g [out_dim] or NULL, b [out_dim]
 *   rowmap [n_rows] : source row of packed row r, -1 = zero row   (n_rows multiple of 32)
 *   colmap [(8+ks_in)*32], colscale [...] : source column of K slot s (-1 = zero) and a factor
 *   wpack_layer : destination (n_rows/32 chunks of (8+ks_in)*2 KiB) or NULL to only write the bias
 *   bias_layer  : destination, MP_BIAS_STRIDE floats (rows >= n_rows are zeroed); bias_scale multiplies (b + hoist).
 * Softplus networks run in scaled units (csrc/mlp_core.hpp): the host passes colscale = K for input-fed slots and
 * bias_scale = K = 100 log2(e) on hidden layers, and colscale = 1/K on the last (linear) layer. */
int mp_pack_layer(const float* v, const float* g, const float* b, int out_dim, int in_dim, const int* rowmap,
                  int n_rows, const int* colmap, const float* colscale, int ks_in, int hoist_col0, int hoist_n,
                  const float* hoist_vec, float bias_scale, void* wpack_layer, float* bias_layer, void* stream);
/* mp_pack_layer for ALL layers of one network in ONE launch (a training forward repacks the sampler's half-precision SDF net of
 * every person: 9 layers x 2 launches each before).  table: n_layers (<= MP_MAX_LAYERS) DEVICE-resident records, one per layer,
 * fields as mp_pack_layer's arguments (device pointers; hoist_vec NULL or hoist_n 0 = no hoisting; wpack_layer NULL = bias
 * only); every layer's bias row is written for all MP_BIAS_STRIDE entries (zeros past n_rows). */
typedef struct {
    const void *v, *g, *b, *rowmap, *colmap, *colscale, *hoist_vec;
    void *wpack_layer, *bias_layer;
    int out_dim, in_dim, n_rows, hoist_col0, hoist_n;
    float bias_scale;
} MpPackLayer;
int mp_pack_layers(const MpPackLayer* table, int n_layers, int ks_in, void* stream);
/* Feature fold.  An SDF network ends in a linear layer W8 [1 + n_feat][in8] (row 0 = sdf, rows 1.. = the feature vector,
 * networks.py:176-181) whose features only feed the first layer Wc [out_c][in_c] of its rendering network, in columns
 * [feat_col0, feat_col0 + n_feat) (networks.py:277-281, 305-311).  That layer is linear in them, so
 *   Wc[:, feat] (W8[1:] h + b8[1:]) = (Wc[:, feat] W8[1:]) h + Wc[:, feat] b8[1:]
 * and the product depends on parameters only.  This writes, in fp32 and with weight norm resolved on both factors (g NULL: none),
 *   out_w [out_c][in_c] : Wc_eff, with columns feat_col0 + k (k < in8 <= n_feat) replaced by sum_f Wc_eff[r][feat_col0 + f] *
 *                         W8_eff[1 + f][k] (zeros for in8 <= k < n_feat): a layer that takes the SDF network's last hidden
 *                         vector where Wc takes the features;
 *   out_b [out_c]       : bc + Wc_eff[:, feat] b8[1:]
 * for mp_pack_layer(s) to pack like any other layer (in scaled units: colscale = 1/K on those columns).  n_feat <= 1024. */
int mp_fold_features(const float* vc, const float* gc, const float* bc, int out_c, int in_c, int feat_col0, int n_feat,
                     const float* v8, const float* g8, const float* b8, int in8, float* out_w, float* out_b, void* stream);

/* ---- fused MLP evaluation -------------------------------------------------------------------
 * mp_mlp_sdf: ImplicitNet.forward restricted to the sdf column (networks.py:126-181; caller:
 * multiply.py:140-141 inside the sampler, ray_sampler.py:85-88).
 *   xc [*][3] canonical points, worklist[i] = point id (NULL: id = i), *count work items
 *   sdf_out[point id] <- sdf.  multires = 6 Fourier encoding of 3-D input.
 * Range: hidden pre-activations are carried as halves in scaled units (x 100 log2 e), so |z| < 65504 / 144.27 = 454.  Beyond
 * that the sdf comes out +-inf or NaN, never finite and wrong (a unit that overflows towards -inf is exact: softplus 0). */
int mp_mlp_sdf(const MpNet* net, const void* wpack, const float* bias, const float* xc, const int* worklist,
               const int* count, int max_count, float* sdf_out, void* stream);

/* mp_mlp_sdf_x2: the same queries with SPLIT ACTIVATIONS (round 6; the sampler's default, `Multiply.sampler_sdf_mode = 'f16x2'`):
 * same arguments, same packed half-precision weights and bias table, but every activation travels as two halves x = hi + lo
 * (22 mantissa bits) and a product is two MFMAs, W_h x_h + W_h x_l, with fp32 accumulation and an fp32 softplus.  The error
 * against the fp32 reference network drops from ~1e-3 to ~1e-4 (what is left is the rounding of the weights), the depths the
 * reference's sampler derives from these values (ray_sampler.py:85-94, multiply.py:137-151) agree accordingly. */
int mp_mlp_sdf_x2(const MpNet* net, const void* wpack, const float* bias, const float* xc, const int* worklist,
                  const int* count, int max_count, float* sdf_out, void* stream);

/* mp_mlp_full: ImplicitNet.forward, all 1+256 outputs, for callers outside the fused renderer
 * (multiply_model.py:941-945 query_oc).  d_in = 3 (multires 6) or 4 (multires 10). out [n][257]. */
int mp_mlp_full(const MpNet* net, const void* wpack, const float* bias, const float* x, int d_in, int n,
                float* out, void* stream);

/* mp_mlp_shade: value + forward-mode tangents of the foreground ImplicitNet, i.e. sdf, d sdf/d x_c and the
 * 256 features in one pass (replaces the second forward + autograd.grad of multiply.py:643-659), then
 * normal = normalize(normalize(grad . Jinv), eps=1e-6) (multiply.py:661, :606).
 *   worklist[i] = point id; xc [*][3]; jinv [*][9] (row-major inverse of d x_d / d x_c)
 *   sdf_out[id], normal_out[id][3]; feat_frag: f16 B-fragments, 512 B per WORK INDEX (consumed by mp_mlp_color) */
int mp_mlp_shade(const MpNet* net, const void* wpack, const float* bias, const float* xc, const float* jinv,
                 const int* worklist, const int* count, int max_count, float* sdf_out, float* normal_out,
                 void* feat_frag, void* stream);

/* mp_mlp_shade_rev: same outputs as mp_mlp_shade, computed in reverse mode, segment by segment of the worklist:
 * a plain forward sweep that writes sigmoid(100 z) of every hidden unit as UNORM8 (mp_sig_bytes_per_point() = 2048 B per work
 * index) into `sig` (seg_points * mp_sig_bytes_per_point() B, seg_points a multiple of 256, ZERO-INITIALISED once by the
 * caller), then a reverse sweep through
 * the TRANSPOSED layers (gnet / gpack: the 'grad' plan of multiply_amd/hip.py; w8_slots: the sdf row of the last layer,
 * 256 halves in K-slot order).  Two network columns per point instead of the four of the forward-mode kernel.
 * Range (as mp_mlp_sdf): a point with a hidden pre-activation beyond |z| = 454 gets a non-finite sdf, and then a non-finite
 * normal too (0 x sdf is added to it: the byte-sized stored sigmoids cannot carry the overflow); mp_mlp_color turns a
 * non-finite normal into a non-finite rgb.  Measured at 1.2x the limit: every output finite inside the range, and non-finite
 * exactly at the points whose sdf is. */
int mp_sig_bytes_per_point(void);
int mp_mlp_shade_rev(const MpNet* net, const void* wpack, const float* bias, const MpNet* gnet, const void* gpack,
                     const void* w8_slots, const float* xc, const float* jinv, const int* worklist, const int* count,
                     int max_count, float* sdf_out, float* normal_out, void* feat_frag, void* sig, int seg_points,
                     void* stream);
/* mp_mlp_shade_rev_fold: mp_mlp_shade_rev without the 256 feature rows of the last layer.  net / wpack / bias: the 'sdf' plan
 * (the network ends in the one-chunk sdf row, as for mp_mlp_sdf; anything else: -1); h7_frag receives, in feat_frag's layout and
 * size, the last hidden layer's activations in scaled units (x 100 log2 e) as f16 B-fragments.  mp_mlp_color turns them into the
 * same colours when its first layer is packed from mp_fold_features' output.  sdf_out and normal_out: the bits of
 * mp_mlp_shade_rev (the same sdf row, K order and accumulator; the reverse sweep does not read the features). */
int mp_mlp_shade_rev_fold(const MpNet* net, const void* wpack, const float* bias, const MpNet* gnet, const void* gpack,
                          const void* w8_slots, const float* xc, const float* jinv, const int* worklist, const int* count,
                          int max_count, float* sdf_out, float* normal_out, void* h7_frag, void* sig, int seg_points,
                          void* stream);

/* mp_mlp_color: RenderingNet.forward mode 'pose_no_view' (networks.py:277-281, 305-311):
 * sigmoid(MLP([x_c, n, lin_pose(pose) (hoisted), feat])) -> rgb_out[id][3].  feat_frag: the features as written by mp_mlp_shade /
 * mp_mlp_shade_rev -- or mp_mlp_shade_rev_fold's h7_frag together with a pack whose first layer is the folded one. */
int mp_mlp_color(const MpNet* net, const void* wpack, const float* bias, const float* xc, const float* normal,
                 const void* feat_frag, const int* worklist, const int* count, int max_count, float* rgb_out,
                 void* stream);

/* mp_background: NeRF++ inverted-sphere background (multiply.py:514-539, 682-726): for every ray, n_bg depths
 * -> depth2pts_outside -> bg ImplicitNet (frame code hoisted) -> bg RenderingNet ('nerf_frame_encoding') ->
 * bg_volume_rendering with AbsDensity -> bg_rgb[R][3].  z_bg [n_bg] are the (shared) inverse depths in
 * DESCENDING order as after the flip of multiply.py:516, or per ray [R][n_bg] if z_per_ray. */
int mp_background(const MpNet* net_imp, const void* wpack_imp, const float* bias_imp, const MpNet* net_ren,
                  const void* wpack_ren, const float* bias_ren, const float* dirs, const float* cam, const float* z_bg,
                  int z_per_ray, int n_rays, float radius, float* bg_rgb, void* stream);
/* mp_background_fold: the same with the feature fold: net_imp is the 'sdf' plan of the background ImplicitNet (it ends in the
 * one-chunk density row; anything else: -1) and net_ren's first layer is packed from mp_fold_features' output, so that it takes
 * the density network's last hidden activations from the registers. */
int mp_background_fold(const MpNet* net_imp, const void* wpack_imp, const float* bias_imp, const MpNet* net_ren,
                       const void* wpack_ren, const float* bias_ren, const float* dirs, const float* cam, const float* z_bg,
                       int z_per_ray, int n_rays, float radius, float* bg_rgb, void* stream);

/* ---- SMPL ------------------------------------------------------------------------------------
 * SMPLServer.forward (lib/model/smpl.py:50-94) -> lbs (lib/smpl/lbs.py:136-229): posed vertices, bone
 * transforms relative to the canonical pose (tfs_c_inv, may be NULL for absolute), posed joints.
 *   params [86] = scale, transl3, thetas72, betas10 (device).  work: >= 3*V + 24*16 + 207 + 64 floats. */
int mp_smpl_pose(const float* v_template, const float* shapedirs, const float* posedirs, const float* j_regressor,
                 const float* lbs_weights, const int* parents, const float* params, const float* tfs_c_inv,
                 float* verts, float* tfs, float* joints, float* work, void* stream);
/* Adjoint of the posed vertices verts = s (sum_j w_j A_j [v_posed; 1] + transl), v_posed = v_shaped + posedirs^T pf
 * (lbs.py:196-221, smpl.py:77-78) for the parameters `params` of an mp_smpl_pose call whose work buffer is `work`
 * (v_shaped, A and pf are read from it; v_posed is recomputed, posedirs is read once).  dverts [V][3].
 * Two launches, no atomics: per-workgroup partials of 32 vertices each into scratch [MP_SMPL_VBWD_SCRATCH], then a
 * finishing pass that sums them in a fixed order (bit-identical results on every call).  Output dlbs [MP_SMPL_DLBS]:
 *   [0, 384)   dA [24][16]: adjoint of the rest-relative transforms A (work layout, unscaled; row 3 = 0)
 *   [384, 591) dpf [207]:   adjoint of the pose feature (R_j - I, j >= 1)
 *   [591, 677) dparams [86]: the direct terms -- d scale, d transl, 0 for thetas, d betas through the shape blend shapes
 * mp_smpl_pose_bwd_lbs turns dA / dpf / dparams into the gradient of the 86 parameters. */
#define MP_SMPL_VBWD_SCRATCH (216 * 512)
#define MP_SMPL_DLBS (24 * 16 + 207 + 86)
int mp_smpl_verts_bwd(const float* posedirs, const float* shapedirs, const float* lbs_weights, const float* params,
                      const float* work, const float* dverts, float* scratch, float* dlbs, void* stream);
/* mp_smpl_pose for N parameter rows params [N][86] against one table set, forward only, in two launches whatever N is (one
 * when verts is NULL): the chain runs one workgroup per row, and the vertex kernel stages each 207 x 96 tile of posedirs once
 * per workgroup and sweeps it over all rows, MP_SMPL_BATCH_ROWS at a time -- posedirs is read once per call, not once per row.
 * Outputs verts [N][V][3], tfs [N][24][16], joints [N][24][3]; each may be NULL to skip it.  tfs_c_inv as in mp_smpl_pose.
 * work: N * MP_SMPL_BATCH_ROW_WORK floats (per row: rest joints [72] at 0, rest-relative transforms [24][16] at 80, pose
 * feature [207] at 464).  The arithmetic per row is mp_smpl_pose's, and a row's operations and their order depend neither on N
 * nor on the row's position: a row has the same bits alone and inside any batch.  No atomics.
 * Status -1 without a launch: N < 0, a NULL table, NULL params / work with N > 0; N == 0 returns 0. */
#define MP_SMPL_BATCH_ROWS 16
#define MP_SMPL_BATCH_ROW_WORK 672
int mp_smpl_pose_batch(const float* v_template, const float* shapedirs, const float* posedirs, const float* j_regressor,
                       const float* lbs_weights, const int* parents, const float* params, int N, const float* tfs_c_inv,
                       float* verts, float* tfs, float* joints, float* work, void* stream);

/* Nearest-neighbour acceleration structure over one vertex set (exact K=1 search, replaces
 * pytorch3d.ops.knn_points, deformer.py:39): vertices gathered in cluster order + bounding spheres.
 *   perm [NC*CL] vertex ids in cluster order (-1 = padding); vsorted [NC*CL][4] = x,y,z,id-as-int-bits;
 *   cbound [NC + NC / 2][4] = centre, radius of every cluster, then of every PAIR of clusters (2c, 2c + 1): the coarse granularity the
 *   training-mode searches of mp_warp_inverse / mp_warp_inverse_shade run on; the other consumers read the first NC rows. */
int mp_knn_build(const float* verts, const int* perm, float* vsorted, float* cbound, void* stream);

/* Oriented box of the posed vertices inflated by `inflate` (multiply.py:208-214; PCA axes instead of trimesh's
 * minimum-volume box).  obb [15] = centre3, axes (3 rows), half extents3. */
int mp_obb(const float* verts, float inflate, float* obb, void* stream);

/* The MINIMUM-VOLUME oriented box the reference asks trimesh for (multiply.py:208-214: smpl_mesh.bounding_box_oriented,
 * primitives.Box(extents * 1.2, transform)) from the convex hull of the posed vertices.  The hull is computed by the caller
 * (multiply_amd/obb.py hull_search_inputs: Qhull); the search over (hull-facet normal, silhouette edge) candidates and the box
 * itself are computed here in fp64.  All inputs fp64, device resident:
 *   hull_verts [H][3]; normals [N][3] the distinct facet normals in the caller's order of preference; per hull edge
 *   edge_vec [E][3] and the normals of its two facets edge_na / edge_nb [E][3]; work [2 N] scratch.
 *   obb [16] as mp_obb: centre3, axes (3 rows: facet normal, rectangle sides), half extents3 x inflate, pad. */
int mp_obb_hull(const double* hull_verts, int n_hull_verts, const double* normals, int n_normals, const double* edge_vec,
                const double* edge_na, const double* edge_nb, int n_edges, float inflate, double* work, float* obb, void* stream);

/* The same box with the convex hull ALSO built on the device (gift wrapping: 8 workgroups on one XCD share the pivots of a
 * level-synchronous front, one of them keeps the edge table; fp64 predicates; ~0.35 ms for a 6 890-vertex body): no device -> host
 * copy of the posed vertices, no host hull.  A BATCH of n_bodies (<= 64) bodies in one call, their wraps side by side:
 * verts [n_bodies][n_verts][3] fp32 (n_verts < 6912); work [n_bodies][mp_obb_hull_device_work_bytes()] bytes, 8-byte aligned;
 * obb [n_bodies][16]; status [n_bodies][8] (device ints): {hull vertices, facets, edges, failed, rounds, pivot / insert / total
 * clocks x 16}: failed != 0 (a non-manifold patch from exactly coplanar vertices, or more than 2048 facets) leaves obb all-zero -- the caller
 * reads it with its other device counts and falls back to mp_obb_hull with a host-side hull. */
int mp_obb_hull_device_work_bytes(void);
int mp_obb_hull_device(const float* verts, int n_verts, int n_bodies, float inflate, void* work, float* obb, int* status, void* stream);
/* Test hook: on != 0 makes every following mp_obb_hull_device call take its give-up path (the wrap's workgroups spin on each other
 * and abandon the wrap after ~30 ms when they are not all resident: status[..][3] = 1, the caller falls back to the host hull).
 * Returns the previous setting. */
int mp_debug_hull_abandon(int on);

/* ---- training objective ---------------------------------------------------------------------
 * The per-ray / per-point terms of Loss.forward (reference code/lib/model/loss.py:6-177) and the gradient of their weighted sum in
 * ONE launch (csrc/loss.hip).  All pointers device fp32 unless noted:
 *   rgb [R][3] (NaN rows are left out), rgb_gt [R][3], acc [R], accp [R][P], gth [N][3] (eikonal gradients),
 *   sam [R][P] SAM logits or NULL (term off), in_mask [R] bytes or NULL (in-shape term off)
 *   -> terms [8] = {total, rgb_loss, eikonal, bce, in_shape, sam_mask, 0, 0} with
 *      total = rgb_loss + w_eik eikonal + w_bce bce + w_in in_shape + w_sam sam_mask   (the caller resolves the epoch schedules)
 *      d_rgb [R][3], d_acc [R], d_accp [R][P], d_gth [N][3] = d total / d (rgb, acc, accp, gth). */
typedef struct {
    const float *rgb, *rgb_gt, *acc, *accp, *gth, *sam;
    const unsigned char* in_mask;
    float *d_rgb, *d_acc, *d_accp, *d_gth, *terms;
    int n_rays, n_persons, n_eik;
    float w_eik, w_bce, w_in, w_sam, eps;
} MpLossArgs;
int mp_loss_fused(const MpLossArgs* args, void* stream);

/* ---- rays -------------------------------------------------------------------------------------
 * rend_util.get_camera_params (lib/utils/rend_util.py:45-87) + far sphere root (:131-147).
 *   uv [R][2], intrinsics [16], pose [16] -> dirs [R][3], far [R]; cam is pose[:3,3]. */
int mp_ray_setup(const float* uv, const float* intrinsics, const float* pose, int n_rays, float radius, float* dirs,
                 float* far, void* stream);
/* Ray / box test and ordered compaction (multiply.py:256-266): hit_index [<=R] ascending ray ids, *hit_count;
 * inv_index [R] = position in hit_index or -1.  group_size: rays of a convergence group without a hit get their
 * first ray as fallback (multiply.py:262-263 applied per chunk). scan_tmp: >= R + ceil(R / 1024) ints (the flags, then one
 * partial sum per scan block of 1024 rays). */
int mp_ray_cull(const float* dirs, const float* pose, const float* obb, int n_rays, int group_size, int* hit_index,
                int* hit_count, int* inv_index, int* scan_tmp, void* stream);
/* The same, refined for eval-mode rendering without changing a pixel: a ray that passes the box but stays further than the
 * outlier radius 0.1 (deformer.py:49) from every vertex on [near, far[r]] carries only sdf = 4 samples (multiply.py:142-143);
 * when 1 - exp(-sigma(4) (far - near)) is exactly 0 in fp32 its pixel is the background's, exactly like a ray outside the
 * box, and it is dropped here.  cbound [MP_KNN_NC][4] = the bounding spheres of the posed vertex clusters (mp_knn_build), far [R]
 * from mp_ray_setup, beta = device scalar (density), near_ = the sampler's near bound. */
int mp_ray_cull_near(const float* dirs, const float* pose, const float* obb, const float* cbound, const float* far,
                     const float* beta, float near_, int n_rays, int group_size, int* hit_index, int* hit_count,
                     int* inv_index, int* scan_tmp, void* stream);
/* Explicit hit set (parity tests): fills hit_count / inv_index from a given ascending hit_index [n_hit]. */
int mp_ray_hits_from_index(const int* hit_index, int n_hit, int n_rays, int* hit_count, int* inv_index, void* stream);

/* ---- canonical warp ---------------------------------------------------------------------------
 * SMPLDeformer.forward(inverse=True) (deformer.py:19-50, 72-88): nearest posed vertex -> its skinning weights ->
 * x_c = (sum_j w_j T_j)^-1 x ; outlier = dist > 0.1.
 * The blended transform only depends on the nearest vertex: mp_blend_table evaluates it once per pose for every vertex,
 * table [n_verts][3][4] fp32, row r = (I[r][0..2], T[r][3] / T[3][3]) with T = sum_j skin_w[v][j] tfs[j], I = T[:3,:3]^-1
 * (skin_w [n_verts][24], tfs [24][16]); the warp kernels read x_c = I (x - c) and jinv = I from it (`blend_table`).
 * Points are either explicit (pts [max_rays][3], dirs, pose, hit_index, hit_count and z unused) or implicit samples of hit rays:
 * point id = k*n_s + s, x = cam + z[k*z_stride + s] * dirs[hit_index[k]], cam = pose[:3,3].
 *   mode 0 (training): every point is written to xc and appended to worklist.
 *   mode 1 (eval): outliers get sdf_out = 4 (multiply.py:142-143) and are NOT appended.
 *   ray_active [max_rays] per-ray flag or NULL; launch_active: device int, 0 = nothing to do (kernel exits), or NULL.  Outputs: xc [n][3], worklist, *work_count (atomic, must be 0). */
int mp_blend_table(const float* skin_w, const float* tfs, int n_verts, float* table, void* stream);
int mp_warp_inverse(const float* pts, const float* dirs, const float* pose, const int* hit_index, const int* hit_count,
                    const float* z, int z_stride, int n_s, int max_rays, const float* vsorted, const float* cbound,
                    const float* blend_table, int mode, const int* ray_active, const int* launch_active,
                    float* xc, unsigned char* outlier, float* sdf_out, int* worklist, int* work_count, void* bin_work,
                    void* stream);
/* bin_work (optional, mode 0 with implicit samples only; mp_warp_bin_work_bytes(max_rays * n_s) bytes, 16-byte aligned): the
 * points are first grouped by their nearest vertex cluster, so that the 64 points of a wave open the same few clusters -- a
 * training batch's random pixels otherwise scatter every wave over the whole body (50 of the then 108 clusters opened per wave).  Results
 * are identical (they go out by point id); only the order of the worklist changes. */
int mp_warp_bin_work_bytes(int n_points);
/* The same for the final samples of the shading pass (z rows hold n_s+1 depths).  eval_mode: outliers get sdf 4 and are
 * dropped from the worklist only when their compositing alpha 1-exp(-sigma(4) dt) is exactly 0 in fp32.
 * need_flag [id] (optional) = 1 for every point that was appended; nn_index [id] (optional) = the nearest posed vertex
 * whose skinning weights were used (the training backward needs it: deformer.py:47 detaches the weights). */
int mp_warp_inverse_shade(const float* dirs, const float* pose, const int* hit_index, const int* hit_count,
                          const float* z, int z_stride, int n_s, int max_rays, const float* vsorted, const float* cbound,
                          const float* blend_table, int eval_mode, const float* beta, float* xc,
                          unsigned char* outlier, unsigned char* need_flag, float* sdf_out, int* worklist,
                          int* work_count, int* nn_index, void* bin_work, void* stream);
/* Jacobian of forward skinning at canonical points (deformer.py:31-35 + multiply.py:625-641): nearest CANONICAL
 * vertex -> weights -> J = (sum_j w_j T_j)[:3,:3] -> jinv [id][9].
 * n_s > 0: points are the samples of the hit rays (id = k*n_s + s, as in mp_warp_inverse_shade) and only ids with
 * need[id] != 0 are processed; n_s == 0: explicit list of n_pts points (need, hit_count ignored).
 * seed [id] (optional, with verts_c [V][3] = the canonical vertices in original order): a vertex id per point whose
 * canonical distance bounds the search (the posed nearest vertex from mp_warp_inverse_shade); the result stays exact. */
int mp_warp_jacobian(const float* xc, const unsigned char* need, const int* hit_count, int max_rays, int n_s, int n_pts,
                     const float* vsorted_c, const float* cbound_c, const float* blend_table, float* jinv,
                     int* nn_index, const int* seed, const float* verts_c, void* stream);

/* ---- VolSDF error-bound sampler (ray_sampler.py:66-220), split at the SDF queries ---------------
 * State per hit ray k (row stride zmax = 640): zs/sdfs sorted samples and their sdf, nz count, znew/sdfnew [128]
 * the samples whose sdf is being queried, beta, done flag.  Per group: not_converged flags.
 * cfg = {N_samples, N_samples_eval, N_samples_extra, beta_iters, max_total_iters} ints, {eps, add_tiny, near} floats.
 * A convergence group = the hit rays whose ray id falls in one block of `group_size` consecutive rays of the call
 * (n_rays_total rays): the reference's `beta.max() > beta0` vote (ray_sampler.py:137) is taken per group, so that a
 * whole-frame call with group_size = pixel_per_batch reproduces the reference's chunked rendering loop exactly. */
typedef struct {
    int n_samples, n_samples_eval, n_samples_extra, beta_iters, max_total_iters;
    float eps, add_tiny, near_;
} MpSamplerCfg;
typedef struct {
    float* zs; float* sdfs; int* nz; float* znew; float* sdfnew; float* beta; int* ray_active;
    int* group_flag;   /* [max_total_iters+1][n_groups] */
    float* zfinal;     /* [max_rays][n_samples + n_samples_extra + 2] */
    int* iters;        /* [n_groups] iterations run (diagnostics) */
    int* any_active;   /* [max_total_iters+1] any_active[i] != 0: some ray still needs SDF queries in iteration i */
} MpSamplerState;
/* uniform start (ray_sampler.py:21-42, 70-76); t_rand [max_rays][n_eval] or NULL (eval: no jitter) */
int mp_sampler_init(const MpSamplerCfg* cfg, const MpSamplerState* st, const float* far, const int* hit_index,
                    const int* hit_count, int max_rays, int group_size, int n_rays_total, const float* t_rand,
                    void* stream);
/* merge the queried samples, d*, error bound, beta bisection, group convergence vote (ray_sampler.py:89-137) */
int mp_sampler_bound(const MpSamplerCfg* cfg, const MpSamplerState* st, const float* beta0, const int* hit_index,
                     const int* hit_count, int max_rays, int group_size, int n_rays_total, int iter, void* stream);
/* up-sample from the error-bound pdf, or draw the final samples and assemble zfinal (ray_sampler.py:139-209);
 * u_final [max_rays][n_samples] / extra_idx [max_total_iters][n_extra] supply the training randomness (row k-1 =
 * randperm(n_eval*k)[:n_extra], used when the sorted list holds n_eval*k depths), NULL = eval linspace */
int mp_sampler_resample(const MpSamplerCfg* cfg, const MpSamplerState* st, const float* beta0, const float* far,
                        const int* hit_index, const int* hit_count, int max_rays, int group_size, int n_rays_total,
                        int iter, const float* u_final, const int* extra_idx, void* stream);

/* ---- compositing (multiply.py:425-480, 544-545, 590) ---------------------------------------------
 * Per ray: merge the persons' samples by t_end (ties: lower person first), Laplace density (density.py:20-29),
 * alpha = 1-exp(-sigma dt), T = exp(-exclusive cumsum), sums; bg transmittance = exclusive T of the last sample.
 *   per person p: inv_index[p] [R], z[p] [*][n_z] (n_z = S+1 depths, last = z_max), sdf[p] [*][S], rgb[p] [*][S][3],
 *   normal[p] [*][S][3]  (pointer tables live in device memory, P entries each)
 * Outputs [R]: fg_rgb[3], normal[3], acc, acc_person[P], bg_T; rgb = fg + bg_T*bg_rgb; fg_out = fg + bg_T.
 * Tie rules: samples of equal t_end merge with the lower person first; hence, when several persons end at the same final
 * depth, the HIGHER person's last sample is the last of the merged list, and bg_T is the transmittance in front of that sample
 * (everything of the other persons and that person's first S-1 samples).  A ray without samples: rgb = bg_rgb, fg_out = 1,
 * normal = 0, acc = 0, bg_T = 1; a person the ray misses (inv_index < 0): exactly 0 in its acc_person column.
 * Zero-weight rule: rgb and normal of a sample are read only where its float32 weight w is not exactly 0 -- the eval path leaves
 * the colours and normals of unshaded samples undefined (they may be NaN), and such samples have fe = 0, hence w = 0.
 * bg_rgb may be NULL: a white background (bg = 1).  Every output pointer is required.  All outputs are stored, rows [0, n_rays)
 * only; no atomics, fixed summation order: bit-identical from run to run.
 * Status: -1 n_person outside [0, 8]; 0 for n_rays <= 0; -2 LDS limit: 4 waves x n_person x (3S+1) floats must fit 160 KiB (at
 * n_person = 8 up to S = 426).  In all three nothing is launched and nothing written. */
int mp_composite(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                 const float* const* sdf, const float* const* rgb, const float* const* normal, const float* beta,
                 const float* bg_rgb, float* rgb_values, float* fg_rgb_values, float* normal_values, float* acc_map,
                 float* acc_person, float* bg_T, void* stream);
/* Geometry of the same merge, from the same tables (no rgb / normal): with ts, te the ends of a sample, tm their mean,
 * fe = sigma (te - ts), E the free energy in front of it in merged order, w = (1-exp(-fe)) exp(-E), and E0 / w0 the same with
 * the person's own samples only ("solo": the person as if rendered alone); L = -ln(1 - level), level in (0,1):
 *   depth [R] = sum w tm (unnormalised, goes with acc_map)          depth_person [R][P] = sum_i w tm (with acc_person)
 *   depth_level [R] = ts + (te-ts) clamp((L-E)/fe, 0, 1) of the FIRST sample in merged order with E + fe >= L (the minimum
 *                     of the key (te, person) over the samples that satisfy it), -1 if none; front_person [R] its column, or -1
 *   acc_solo [R][P] = sum_i w0    depth_solo [R][P] = sum_i w0 tm    depth_solo_level [R][P]: the level rule on person n alone
 * Depths are distances along the ray in the units of z; rays a person does not hit give 0 / -1 in its column.  Any output
 * pointer may be NULL (skipped).  No atomics, fixed summation order: bit-identical from run to run.
 * Status: -1 n_person > 8, -2 LDS limit, -3 level outside (0,1) (no launch), 0 for n_rays <= 0. */
int mp_composite_geometry(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                          const float* const* sdf, const float* beta, float level, float* depth, float* depth_person,
                          float* depth_level, int* front_person, float* acc_solo, float* depth_solo,
                          float* depth_solo_level, void* stream);


/* ---- fp32 training path (layer-wise forward with stash + hand-written backward) ----------------------------------
 * The reference trains in fp32 through torch autograd (multiply_model.py:192-217).  These entry points are the pieces of
 * the same computation as explicit forward / adjoint kernels; multiply_amd/train.py chains them inside one
 * torch.autograd.Function so that the reference's Loss and optimisers work unchanged.
 * Forward-mode row convention: a tensor of a network evaluated for P points with spatial tangents has 4P rows:
 * [0,P) values, [P,2P) d/dx, [2P,3P) d/dy, [3P,4P) d/dz.  "ld*" are row strides in floats.
 * Empty problems: every mp_tr_* entry point returns 0 and launches NOTHING (no pointer is read, all may be NULL) when its
 * problem has no elements -- rows, n, P, E, n_pts, R, n_verts, out_dim or C <= 0, whichever it takes (for a product such as
 * rows x C: either factor).  Three entry points still have an output with one factor empty and write it: mp_tr_colsum with
 * rows <= 0 and mp_tr_bg_comp_fwd with NBG <= 0 store zeros, mp_tr_hoist_fwd with n <= 0 copies b. */
/* C[M,N] (+)= A[M,K] . B[N,K]^T (+ bias[N] on rows < bias_rows) (optional ReLU); exact-fp32 MFMA */
int mp_gemm_nt(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
               const float* bias, int bias_rows, int accumulate, int relu, void* stream);
/* The same product with every fp32 operand split into two bfloat16 halves (x = hi + lo) on its way into LDS and three
 * v_mfma_f32_16x16x32_bf16 per block product (hi.hi + hi.lo + lo.hi), fp32 accumulate: relative error ~2^-16 per product,
 * fp32 range; same arguments and epilogue. */
int mp_gemm_nt_bf16x3(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
               const float* bias, int bias_rows, int accumulate, int relu, void* stream);
/* C[M,N] += A[K,M]^T . B[K,N]  (C must be initialised; fp32 atomics) */
int mp_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* colsum,
               int colsum_rows, void* stream);
/* The same contraction on the split-bf16 path (see mp_gemm_nt_bf16x3); the 4 x 4 register transposition that turns the row-major
 * operands into k-contiguous MFMA fragments happens on the way into LDS.  colsum stays an exact fp32 sum. */
int mp_gemm_tn_bf16x3(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* colsum,
               int colsum_rows, void* stream);
/* Up to MP_TN_MAX_GROUPS such contractions in ONE launch (the weight gradients of all layers of a network): groups is a HOST
 * array; every group needs 16-byte aligned A, B, lda / ldb multiples of 4 and M, N multiples of 128.  Far fewer row slices per
 * output than one launch per contraction needs to fill the chip, hence far fewer fp32 atomics.
 * Status (the arguments are checked before anything is launched, so a non-zero argument status means NO group was computed):
 *    0  launched (or n_groups <= 0: nothing to do);  > 0: the launch's hipError_t
 *   -1  n_groups > MP_TN_MAX_GROUPS (the caller cuts its list: train.gemm_tn_grouped)
 *   -2  a group the kernels do not take: M or N no positive multiple of 128, lda or ldb no multiple of 4, A or B not 16-byte
 *       aligned, or an EMPTY contraction, K <= 0.  Unlike mp_gemm_tn[_bf16x3], which return 0 without a launch for K <= 0, an
 *       empty group is refused and not skipped: every caller contracts over a person's sample rows plus its eikonal points or
 *       over all background samples, never zero rows, so an empty record is a caller's bug and not a case to pass over.
 * C, colsum and ldc carry no alignment requirement; two groups of one call may add into the same C. */
#define MP_TN_MAX_GROUPS 24
typedef struct {
    const float* A;
    const float* B;
    float* C;
    float* colsum;       /* may be NULL */
    int lda, ldb, ldc, M, N, K, colsum_rows, pad_;
} MpTnGroup;
int mp_gemm_tn_bf16x3_grouped(const MpTnGroup* groups, int n_groups, void* stream);
/* DETERMINISTIC forms of the three contractions (the training path's opt-in deterministic mode): the same kernels, but every row
 * slice STORES its partial tile into a caller-provided workspace ws [slice][Mp][Np] (Mp, Np = M, N rounded up to 128; a grouped
 * call: group after group) and its column sums into [slice][Mp] behind it; a finishing kernel then adds the slices of every element
 * in ascending slice order and does one C += sum (colsum likewise).  No atomic anywhere: the result is a function of the operands
 * and the shape alone.  The slice plan is the atomic forms' (shape and compile-time constants only).  Groups of one call that add
 * into the same C (same pointer; M, N, ldc must then agree) or the same colsum are added in the order of the groups; C matrices that
 * overlap in any other way are not supported.  The library allocates nothing: *bytes of the size queries (host pointers; bf16x3 != 0:
 * the split-bf16 entry point's plan) is what ws must hold, 16-byte aligned; ws may be reused by the next call on the same stream.
 * Status as above, and -3: ws is NULL, misaligned or smaller than the query's answer (nothing launched). */
int mp_gemm_tn_ws_bytes(int M, int N, int K, int bf16x3, long long* bytes);
int mp_gemm_tn_grouped_ws_bytes(const MpTnGroup* groups, int n_groups, long long* bytes);
int mp_gemm_tn_det(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* colsum,
               int colsum_rows, float* ws, long long ws_bytes, void* stream);
int mp_gemm_tn_bf16x3_det(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K, float* colsum,
               int colsum_rows, float* ws, long long ws_bytes, void* stream);
int mp_gemm_tn_bf16x3_grouped_det(const MpTnGroup* groups, int n_groups, float* ws, long long ws_bytes, void* stream);
/* Fourier features (embedders.py) of x [P][d_in] (d_in 3|4, L octaves) times `scale` into out[.][ld] at col0; fwd != 0 also
 * writes the three (d_in = 3) tangent row blocks */
int mp_tr_pe(const float* x, int d_in, int P, int L, int fwd, float scale, float* out, int ld, int col0, void* stream);
/* nn.Softplus(beta=100) layer on Z [rows][C] -> H at col0 (times scale); P > 0: forward mode (rows = 4P) */
int mp_tr_softplus_fwd(const float* Z, int ldz, int rows, int C, int P, float scale, float* H, int ldh, int col0,
                       void* stream);
int mp_tr_softplus_bwd(const float* Z, int ldz, int rows, int C, int P, float scale, const float* dH, int ldh, int col0,
                       float* dZ, int lddz, void* stream);
int mp_tr_relu_bwd(const float* H, int ldh, int rows, int C, const float* dH, int lddh, float* dZ, int lddz, void* stream);
/* last ImplicitNet layer Z8 [4P][257] -> sdf, normals (multiply.py:606,661) and the colour-net input XA [n][6] = [x_c, n];
 * the adjoint writes column 0 of a zero-initialised dZ8 (d sdf on value rows, d grad on tangent rows).
 * grad / dgrad (optional, [P][3]): d sdf / d x given separately instead of as tangent rows (reverse-over-reverse net); with them
 * Z8 / dZ8 may be NULL (the fused SDF kernels hand sdf / d sdf over as vectors: sdf_out is then not written, dsdf not copied) */
int mp_tr_shade_in_fwd(const float* Z8, int P, int n_pts, const float* xc, const float* jinv, float* XR, float* nrm,
                       float* sdf, const float* grad, void* stream);
int mp_tr_shade_in_bwd(const float* Z8, int P, int n_pts, const float* jinv, const float* dXR, const float* dsdf,
                       const float* dnrm_extra, float* dZ8, float* djinv, const float* grad, float* dgrad, void* stream);
/* eikonal samples (multiply.py:322-331): grad_theta [E][3] = d sdf/dx of points e0..e0+E of the batch */
int mp_tr_eik_fwd(const float* Z8, int P, int e0, int E, float* grad_theta, const float* grad, void* stream);
int mp_tr_eik_bwd(int P, int e0, int E, const float* dgrad_theta, float* dZ8, float* dgrad, void* stream);
int mp_tr_sigmoid_fwd(const float* Z, long long n, float* Y, void* stream);
int mp_tr_sigmoid_bwd(const float* Y, const float* dY, long long n, float* dZ, void* stream);
/* weight norm w = g v/|v| (networks.py:82-83): W [out][in] and its transpose WT [in][out]; adjoint dW -> dv, dg */
int mp_tr_wn_fwd(const float* v, const float* g, int out_dim, int in_dim, float* W, float* WT, void* stream);
int mp_tr_wn_bwd(const float* v, const float* g, int out_dim, int in_dim, const float* dW, float* dv, float* dg,
                 void* stream);
/* The same for many layers in ONE launch each: descs = DEVICE array of n_desc records, rows of all layers concatenated (row0 =
 * first row of a layer in that range, ascending; total_rows = their sum).  fwd reads v, g (NULL: plain weight) and writes W, WT
 * (WT may be NULL); bwd reads v, g and dW = acc_base + dW_off and writes dv = grad_base + dv_off, dg = grad_base + dg_off
 * (offsets in floats: the per-iteration accumulator / gradient buffers move, the table does not). */
typedef struct {
    const float* v;
    const float* g;
    float* W;
    float* WT;
    long long dW_off, dv_off, dg_off;
    int out_dim, in_dim, row0, pad_;
} MpWnDesc;
int mp_tr_wn_fwd_multi(const MpWnDesc* descs, int n_desc, int total_rows, void* stream);
int mp_tr_wn_bwd_multi(const MpWnDesc* descs, int n_desc, int total_rows, const float* acc_base, float* grad_base, void* stream);
/* per-call constant conditioning folded into the bias: b2 = b + W[:, c0:c0+n] vec ; adjoint dW[:, c0:c0+n] += db2 vec^T */
int mp_tr_hoist_fwd(const float* W, int out_dim, int in_dim, const float* b, int c0, int n, const float* vec, float* b2,
                    void* stream);
int mp_tr_hoist_bwd(const float* db2, int out_dim, int in_dim, int c0, int n, const float* vec, float* dW, void* stream);
int mp_tr_colsum(const float* dZ, int ld, int rows, int C, float* db, void* stream);
/* adjoint of mp_composite: d rgb_values / d acc_map / d acc_person -> d sdf[p], d rgb[p], d bg_rgb, d beta (z is a constant).
 * With dC / dA / dA_p the ray's upstream gradients, dw_j = dC . rgb_j + dA + dA_p(j), dT_bg = dC . bg, in merged order:
 *   dfe_j = dw_j T_j e^-fe_j - sum_{i behind j} dw_i w_i - [j is not the very last sample] dT_bg T_bg
 *   d rgb_j = w_j dC,  d bg_rgb = T_bg dC,  d sigma_j = dfe_j (te-ts)_j -> d sdf, d beta through the Laplace density.
 * The merge, both tie rules and T_bg are mp_composite's: the very last sample is the last one of the person whose final depth is
 * the largest, of the HIGHER person on a tie.
 * Store or accumulate: d_sdf[p] and d_rgb[p] are STORED, for every sample of every row that a ray below n_rays refers to; rows of
 * persons a ray misses, rows no such ray refers to and everything past the person's table are not touched.  d_bg_rgb rows
 * [0, n_rays) are stored (T_bg = 1 on a ray without samples).  d_beta ACCUMULATES (+=: one float32 atomic add per ray).
 * NULL: bg_rgb (white background), d_acc, d_acc_person (term dropped), d_bg_rgb (not written).  d_rgb_values is required.
 * Colours: unlike mp_composite this kernel reads the rgb of EVERY sample of a hit row, whatever its weight: dw_j w_j with an
 * undefined (NaN) colour at a zero-weight sample would poison the ray.  Its one caller is the training step, which shades every
 * sample of every hit row (train.py: the colour evaluator runs on all Rp*S points), so every colour is defined there; tables
 * from the eval path, whose unshaded samples carry no colour, must not be handed to it.
 * Launch shape: 4 waves per block, halved down to 1 until n_person x (5S+2) floats per wave fit 160 KiB of LDS (at n_person = 8:
 * 2 waves from S = 256, 1 wave from S = 512).
 * Status: -1 n_person outside [0, 8]; 0 for n_rays <= 0; -2 LDS limit: one wave does not fit.  In all three nothing is launched
 * and nothing written. */
int mp_tr_composite_bwd(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                        const float* const* sdf, const float* const* rgb, const float* beta, const float* bg_rgb,
                        const float* d_rgb_values, const float* d_acc, const float* d_acc_person, float* const* d_sdf,
                        float* const* d_rgb, float* d_bg_rgb, float* d_beta, void* stream);
/* adjoint of mp_composite_geometry's differentiable outputs w.r.t. sdf and beta (z is a constant, as in mp_tr_composite_bwd):
 * d_sdf[p] += , d_beta += .  Any upstream pointer may be NULL (term skipped); all NULL: returns 0, no launch.
 * In mp_composite_geometry's notation (Es / w0 = E / w in the person's own list), for sample j of person p on ray r:
 *   merged sums, dw_i = (d_depth[r] + d_depth_person[r][p(i)]) tm_i :  dfe_j += dw_j e^-E_j e^-fe_j - sum_{i behind j, merged} dw_i w_i
 *   solo sums,  dws_i = d_acc_solo[r][p] + d_depth_solo[r][p] tm_i  :  dfe_j += dws_j e^-Es_j e^-fe_j - sum_{i>j, same person} dws_i w0_i
 *   solo level depth, j* = the crossing sample the forward selects, f = (L-Es_j*)/fe_j*, g = d_depth_solo_level[r][p]; if fe_j* > 0
 *   and 0 < f < 1:  dfe_i -= g (te-ts)_j* / fe_j* for i < j* of that person, dfe_j* -= g (te-ts)_j* / fe_j* f ; else nothing (no
 *   crossing, clamped end).   d sigma_j = dfe_j (te-ts)_j -> d sdf, d beta through the Laplace density.
 * depth_level / front_person (the merged crossing) have no adjoint.  The kernel accumulates: launch it after mp_tr_composite_bwd
 * (which stores) on the same stream; rows of persons a ray misses and rows past the person's table are not touched.
 * Status: -1 n_person > 8, -2 LDS limit, -3 level outside (0,1) (no launch), 0 for n_rays <= 0. */
int mp_tr_composite_geometry_bwd(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                                 const float* const* sdf, const float* beta, float level,
                                 const float* d_depth /*[R]*/, const float* d_depth_person /*[R][P]*/,
                                 const float* d_acc_solo /*[R][P]*/, const float* d_depth_solo /*[R][P]*/,
                                 const float* d_depth_solo_level /*[R][P]*/,
                                 float* const* d_sdf, float* d_beta, void* stream);
/* DETERMINISTIC forms of the two adjoints: every ray's wave STORES its own d beta sum into d_beta_part [n_rays] (the caller's
 * scratch) and a finishing kernel adds them in a fixed order (thread t of 256: rays t, t + 256, .. ascending; then the 256 sums
 * ascending) into d_beta (+=).  Everything else as above (d sdf / d rgb never went through atomics: they are bit-equal to the plain
 * forms').  -3: d_beta_part is NULL (checked after the other status codes: n_rays <= 0 still gives 0). */
int mp_tr_composite_bwd_det(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                            const float* const* sdf, const float* const* rgb, const float* beta, const float* bg_rgb,
                            const float* d_rgb_values, const float* d_acc, const float* d_acc_person, float* const* d_sdf,
                            float* const* d_rgb, float* d_bg_rgb, float* d_beta, float* d_beta_part, void* stream);
int mp_tr_composite_geometry_bwd_det(int n_rays, int n_person, int n_z, const int* const* inv_index, const float* const* z,
                                     const float* const* sdf, const float* beta, float level, const float* d_depth,
                                     const float* d_depth_person, const float* d_acc_solo, const float* d_depth_solo,
                                     const float* d_depth_solo_level, float* const* d_sdf, float* d_beta, float* d_beta_part,
                                     void* stream);
/* background branch pieces (multiply.py:682-726) with per-ray depths zbg [R][NBG] */
int mp_tr_bg_points(const float* dirs, const float* cam, const float* zbg, int R, int NBG, float radius, float* pts,
                    void* stream);
int mp_tr_bg_comp_fwd(const float* sdf, const float* rgb, const float* zbg, int R, int NBG, float* out, void* stream);
int mp_tr_bg_comp_bwd(const float* sdf, const float* rgb, const float* zbg, int R, int NBG, const float* dout, float* dsdf,
                      float* drgb, void* stream);
/* pose optimisation (the reference back-propagates into BodyModelParams: smpl_pose / smpl_trans / smpl_shape):
 *   mp_tr_pe_bwd    : adjoint of the Fourier features (value + tangent rows) w.r.t. the point, dx [P][d_in] +=
 *   mp_tr_warp_bwd  : adjoint of x_c = (sum_j w_j tfs_j)^-1 x and of Jinv w.r.t. tfs (deformer.py:19-50, 72-88; the
 *                     skinning weights of the nearest posed / canonical vertex are constants), dtfs [24][16] +=
 *   mp_smpl_pose_bwd: adjoint of SMPLServer.forward's smpl_tfs (smpl.py:50-94, lbs.py:276-377) w.r.t. the 86 parameters
 *                     [scale, transl 3, thetas 72, betas 10] (betas through the rest joints only: j_shapedirs
 *                     [24][3][10] = J_regressor . shapedirs, or NULL); rest_joints [24][3] of the forward call */
int mp_tr_pe_bwd(const float* x, int d_in, int P, int L, int fwd, const float* dIN, int ld, float* dx, void* stream);
int mp_tr_warp_bwd(const float* xc, const float* dxc, const float* jinv, const float* djinv, const int* nn_posed,
                   const int* nn_cano, int n, const float* skin_w, const float* tfs, float* dtfs, void* stream);
/* DETERMINISTIC form: the points in fixed runs (a function of n), each entry of the 24 x 12 table accumulated by one thread over
 * its run's points in ascending order, one partial table per run into part (floats: the size query's answer, a host pointer),
 * then the tables added in ascending order into dtfs (+=).  -3: part is NULL. */
int mp_tr_warp_bwd_part_floats(int n, long long* floats);
int mp_tr_warp_bwd_det(const float* xc, const float* dxc, const float* jinv, const float* djinv, const int* nn_posed,
                       const int* nn_cano, int n, const float* skin_w, const float* tfs, float* dtfs, float* part, void* stream);
int mp_smpl_pose_bwd(const int* parents, const float* params, const float* tfs_c_inv, const float* rest_joints,
                     const float* j_shapedirs, const float* dtfs, float* dparams, void* stream);
/*   mp_smpl_pose_bwd_lbs: the same chain adjoint with every upstream of SMPLServer.forward: dtfs [24][16] (smpl_tfs),
 *                     dA [24][16] (the rest-relative transforms, mp_smpl_verts_bwd), djoints [24][3] (smpl_jnts),
 *                     dpf [207] (the pose feature, mp_smpl_verts_bwd), dparams_in [86] (added to the result; must not alias
 *                     dparams); any of them NULL = zero.  mp_smpl_pose_bwd is the case dA = djoints = dpf = dparams_in = NULL. */
int mp_smpl_pose_bwd_lbs(const int* parents, const float* params, const float* tfs_c_inv, const float* rest_joints,
                         const float* j_shapedirs, const float* dtfs, const float* dA, const float* djoints,
                         const float* dpf, const float* dparams_in, float* dparams, void* stream);
/* adjoint of x_c = I_nn (x - c_nn) w.r.t. the explicit points x of mp_warp_inverse, gathered onto the vertices they were
 * drawn from: dverts [n_verts][3] += sum over {s : idx[s] == v} of jinv_s^T dxc_s (jinv [n][9] = I_nn row-major, as
 * mp_warp_jacobian writes it).  One thread per vertex, samples in ascending order: deterministic, no atomics. */
int mp_tr_gather_bwd(const int* idx, int n, const float* jinv, const float* dxc, int n_verts, float* dverts, void* stream);
/* reverse-over-reverse SDF net (train.py ImplicitTrainRev): V = sigma'(Z) (.) U (U NULL: the row vector wrow) ;
 * its adjoint (dU, d sigma') ; dZ = sigma' dX scale + sigma'' dS ; Fourier-feature Jacobian products (3-D points). */
int mp_tr_sigmul(const float* Z, int ldz, long long rows, int C, const float* U, int ldu, const float* wrow, float scale,
                 float* V, int ldv, void* stream);
int mp_tr_rev_adj(const float* Z, int ldz, long long rows, int C, const float* U, int ldu, const float* wrow, float uscale,
                  const float* dV, int lddv, float* dU, int lddu, float* dS, int ldds, void* stream);
int mp_tr_dz(const float* Z, int ldz, long long rows, int C, const float* dX, int lddx, float scale, const float* dS, int ldds,
             float* dZ, int lddz, void* stream);
int mp_tr_pe_grad_fwd(const float* x, int P, int L, const float* G, int ldg, float* grad, void* stream);
int mp_tr_pe_grad_bwd(const float* x, int P, int L, const float* dgrad, const float* G, int ldg, float* dG, int lddg,
                      float* dx, void* stream);
int mp_tr_copy_cols(const float* src, int lds, int c0s, float* dst, int ldd, int c0d, long long rows, int C, float scale,
                    int accumulate, void* stream);

/* ---- layer-FUSED training kernels of the foreground ImplicitNet (csrc/tfuse.hip) -----------------------------------------
 * Replace, for the shipped network shape (8 x 256 softplus layers, skip connection into layer 4, 39 Fourier features, 257
 * outputs), the per-layer GEMM + element-wise chain of the reverse-over-reverse SDF net (networks.py:160-181 under
 * autograd with create_graph, multiply.py:620-661): a workgroup keeps 128 points on chip across the whole layer chain
 * (activations = MFMA B operands in registers, split-bf16 weights through an LDS ring by DMA) and writes only what the
 * weight-gradient contractions (mp_gemm_tn_bf16x3) and the adjoint sweep read back.
 *   mp_tf_sdf_pack : W[9] (effective fp32 weights, row-major [out][in]: in = 108 for layer 0, 256 otherwise), B[9] (biases;
 *                    B[0] = layer 0's bias with the conditioning hoisted in) -> wpack (pack_bytes of mp_tf_sdf_sizes: split
 *                    bf16 fragment tiles of W_l, W_l^T in consumption order) and bias_all [9][288] (pack-row order).
 *                    W and B are device arrays of 9 device pointers.
 *   arena          : floats as reported by mp_tf_sdf_sizes(P, &arena_floats, &pack_bytes).  Every [P][256] tensor has P + 1 rows
 *                    (row P: where the lanes of the last tile's missing points store); R1 = (P + 1) 256:
 *                      dZ(l) l=0..7 at l R1 (bwd)          V(l)  l=0..7 at (8+l) R1 (fwd)
 *                      X(l)  l=1..8 at (15+l) R1 (fwd: layer l's input)   dT(l) l=1..7 at (23+l) R1 (bwd)
 *                      U(l)  l=0..6 at (31+l) R1 ;  dS(l) l=0..7 at (38+l) R1
 *                      IN [P][39] at 46 R1 (Fourier features: caller, before fwd), dG [P][39] at 46 R1 + 39 P (caller, before bwd),
 *                      G [P][39] at 46 R1 + 78 P: d sdf / d Fourier features (fwd); then 256 floats the kernels scribble on
 *                    columns >= 217 of X_4 and dT_4 (the re-injected Fourier features of the skip connection, times 1/sqrt 2)
 *                    are NOT written by the kernels: the caller copies them from IN / dG (mp_tr_copy_cols).
 *                    Weight gradients (mp_gemm_tn_bf16x3[_grouped]): dW_l += dZ_l^T X_l + V_l^T dT_l.
 *   mp_tf_sdf_fwd  : feat [P+1][256] and sdf [P+1] (one pad row each) = the last layer's outputs (the reference's column 0 = sdf, columns 1.. = features),
 *                    G, and the stashes
 *   mp_tf_sdf_bwd  : dfeat [P][256], dsdf [P] (adjoints of feat / sdf), dG in BB0 -> dZ_l, dT_l stashes;
 *                    dw8 [256] += gradient of the last layer's sdf ROW (the gradient sweep's V_7 = sigma'_7 (.) w8 and the value
 *                    sweep's sum of d sdf . X_8), db8 [1] += gradient of its sdf BIAS */
int mp_tf_sdf_sizes(int P, long long* arena_floats, long long* pack_bytes);
int mp_tf_sdf_pack(const float* const* W, const float* const* B, void* wpack, float* bias_all, void* stream);
int mp_tf_sdf_fwd(const void* wpack, const float* bias_all, const float* w8, float* arena, int P, float* feat, float* sdf,
                  void* stream);
int mp_tf_sdf_bwd(const void* wpack, const float* w8, float* arena, int P, const float* dfeat, const float* dsdf, float* dw8,
                  float* db8, void* stream);
/* mp_tf_sdf_dx: the adjoint of the input POINTS (pose optimisation) from the stash mp_tf_sdf_bwd has left in `arena`:
 *   dx [P][3] += J_PE(x)^T ( dZ(0) W0[:, 0:39] + (1/sqrt 2) dZ(4) W4[:, 217:256] )
 * W0 / W4 = the effective fp32 weights of layers 0 and 4, row-major [256][ldw0 >= 39] / [256][ldw4 >= 256] (the Fourier columns
 * come first in layer 0 and last in layer 4, where the skip connection re-injects them); x [P][3] the points of the forward
 * call.  ACCUMULATES: the caller has put the gradient sweep's second-order share there (mp_tr_pe_grad_bwd's dx).  Exact fp32
 * (one rounding per product, fp32 accumulation in a fixed order: bit-identical from launch to launch), no atomics; the 39
 * intermediate values never reach memory and the pad rows of the stash are never read.  Reads the stash only: its order
 * against the weight-gradient contractions is free.  P <= 0: nothing to do, returns 0; ldw0 < 39 or ldw4 < 256 (a row too
 * short to hold the Fourier columns): returns -1 without a launch. */
int mp_tf_sdf_dx(const float* arena, int P, const float* W0, int ldw0, const float* W4, int ldw4, const float* x,
                 float* dx, void* stream);
/* mp_tf_sdf_val: the VALUE sweep alone, sdf column only, nothing stashed -- mp_mlp_sdf's interface (worklist of point ids or NULL,
 * device-side count or NULL, sdf_out written at the point ids) at the training path's arithmetic: split-bfloat16 products, fp32
 * accumulation, fp32 softplus, Fourier features from sinf / cosf.  The sampler's queries with `Multiply.sampler_sdf_mode = 'bf16x3'`
 * (ray_sampler.py:85-88): the depths then agree with the fp32 reference to 1e-3 instead of 2e-2 (profiles/r05_sampler_precision.txt).
 * wpack / bias_all as written by mp_tf_sdf_pack (bias row 0 with the call's conditioning hoisted in). */
int mp_tf_sdf_val(const void* wpack, const float* bias_all, const float* xc, const int* worklist, const int* count, int max_count,
                  float* sdf_out, void* stream);

/* The NeRF++ BACKGROUND ImplicitNet (networks.py:126-208 as configured by confs/model: d_in 4, multires 10 -> 84 Fourier features,
 * the frame code hoisted into layer 0's bias, 8 x 256 softplus, skip at layer 4 = [172 | 84] / sqrt 2, 257 outputs, no weight norm;
 * caller multiply.py:514-541) on the same layer-fused skeleton, VALUE ONLY (its outputs feed the density and the colour net; no
 * spatial gradient is taken): mp_tf_bg_fwd = the value sweep, mp_tf_bg_bwd = its adjoint w.r.t. the activations.
 *   mp_tf_bg_pack : W[9] effective weights ([256][116], [256][256] x 2, [172][256], [256][256] x 4, [257][256]), B[9] (B[0] with the
 *                   frame code hoisted in) -> wpack (mp_tf_bg_sizes' pack_bytes), bias_all [9][288]
 *   arena         : R1 = (P + 1) 256 floats per [P][256] tensor (one pad row):  dZ(l) l = 0..7 at l R1 (bwd) | X(l) l = 1..8 at
 *                   (7 + l) R1 (fwd: layer l's input; columns 172.. of X(4) are the caller's: the re-injected features times
 *                   1/sqrt 2, mp_tr_copy_cols) | IN [P][84] at 16 R1 (the Fourier features: caller, before fwd)
 *   mp_tf_bg_fwd  : feat [P+1][256], sdf [P+1] (pad rows) = the last layer's outputs, and the X stashes
 *   mp_tf_bg_bwd  : dfeat [P][256], dsdf [P] -> the dZ stashes; dw8 [256] += the sdf row's weight gradient, db8 [1] += its bias'
 *   weight gradients (caller, mp_gemm_tn_bf16x3[_grouped]): dW_l += dZ_l^T X_l  (l = 0: X = IN; biases = column sums of dZ_l). */
int mp_tf_bg_sizes(int P, long long* arena_floats, long long* pack_bytes);
int mp_tf_bg_pack(const float* const* W, const float* const* B, void* wpack, float* bias_all, void* stream);
int mp_tf_bg_fwd(const void* wpack, const float* bias_all, float* arena, int P, float* feat, float* sdf, void* stream);
int mp_tf_bg_bwd(const void* wpack, const float* w8, float* arena, int P, const float* dfeat, const float* dsdf, float* dw8,
                 float* db8, void* stream);
/* DETERMINISTIC forms of the two backward launches (same stashes, same arithmetic): the last layer's 256 + 1 sums go through one
 * LDS block per wave, added in wave order; every workgroup (= tile of 128 points) STORES its row of part, and finishing launches
 * add the rows in ascending order (beyond 64 tiles: runs of 64 rows first, then the runs) into dw8 / db8 (+=).  part: the size
 * query's floats (a host pointer) for the call's P.  -3: part is NULL. */
int mp_tf_bwd_part_floats(int P, long long* floats);
int mp_tf_sdf_bwd_det(const void* wpack, const float* w8, float* arena, int P, const float* dfeat, const float* dsdf, float* dw8,
                      float* db8, float* part, void* stream);
int mp_tf_bg_bwd_det(const void* wpack, const float* w8, float* arena, int P, const float* dfeat, const float* dsdf, float* dw8,
                     float* db8, float* part, void* stream);

/* The foreground RenderingNet ('pose_no_view', networks.py:263-312: 270 -> 4 x 256 ReLU -> 3, sigmoid) on the same skeleton:
 *   mp_tf_col_pack : W[5] (effective weights, layer 0 = [256][270]: columns 0..5 x_c / normal, 6..13 pose embedding, 14.. features),
 *                    B[5] (B[0] with the pose embedding hoisted in) -> wpack, bias_all [5][288]
 *   stash          : mp_tf_col_sizes floats; N1 = (n + 1) 256 (pad rows as above): H(l) l=0..3 at l N1 (ReLU outputs), dZ(l) l=0..3 at
 *                    (4+l) N1 (their adjoints)
 *   mp_tf_col_fwd  : feat [n][256] (row stride 256), xa [n][6] -> rgb [n][3], H stashes
 *   mp_tf_col_bwd  : drgb, rgb [n][3], w4 = W_4 [3][256] -> dfeat [n][256], dxa [n][6], dz4 [n][3] (adjoint of the last layer's
 *                    pre-activations), dZ stashes.  Weight gradients: dW_l = dZ_l^T H_{l-1} etc. by mp_gemm_tn_bf16x3. */
int mp_tf_col_sizes(int n, long long* stash_floats, long long* pack_bytes);
int mp_tf_col_pack(const float* const* W, const float* const* B, void* wpack, float* bias_all, void* stream);
int mp_tf_col_fwd(const void* wpack, const float* bias_all, float* stash, const float* feat, const float* xa, int n, float* rgb,
                  void* stream);
int mp_tf_col_bwd(const void* wpack, float* stash, const float* w4, const float* rgb, const float* drgb, int n, float* dfeat,
                  float* dxa, float* dz4, void* stream);

/* ---- in / off-surface flags (multiply.py:153-167; training, current_epoch < 250) -------------------------------
 * signed distance of canonical points to a triangle mesh given as face_verts [F][3][3] (= mesh_face_vertices_list[p]):
 * |d| = distance to the closest triangle, negative inside (ray-casting parity), then per ray (n_s consecutive points)
 * off = min > threshold, in = min <= 0.  kaolin 0.13 in the reference (third party): restated, see csrc/mesh.hip. */
int mp_mesh_signed_distance(const float* pts, int n, const float* face_verts, int n_faces, float* sdist, void* stream);
int mp_mesh_ray_flags(const float* sdist, int n_rays, int n_s, float threshold, unsigned char* off, unsigned char* in,
                      void* stream);

/* ---- face index for the same signed distance (csrc/mesh_index.hip): a tree of boxes over the faces in Hilbert-curve order, leaves of 8
 * faces.  mp_mesh_index_signed_distance returns exactly what mp_mesh_signed_distance returns (same per-face arithmetic, faces
 * skipped only when they can neither lower the minimum nor cross the ray, with slack for fp32 rounding), in sub-linear time per
 * point.  Built on the device in three steps, no host synchronisation:
 *   mp_mesh_index_bytes           : size of `index` for n_faces faces (a value, not a status; 16-byte aligned buffer)
 *   mp_mesh_index_keys            : box of all vertices -> index header; keys [n_faces] ints = 30-bit Hilbert-curve key of each centroid
 *   (caller)                      : order [n_faces] 64-bit ints = the permutation that sorts the keys (torch.sort indices)
 *   mp_mesh_index_build           : faces gathered in that order, leaf boxes, inner levels bottom-up
 *   mp_mesh_index_signed_distance : sdist [n]; visits (optional) [n][2] ints = boxes tested, faces evaluated by each point */
int mp_mesh_index_bytes(int n_faces);
int mp_mesh_index_keys(const float* face_verts, int n_faces, void* index, int* keys, void* stream);
int mp_mesh_index_build(const float* face_verts, int n_faces, const long long* order, void* index, void* stream);
int mp_mesh_index_signed_distance(const float* pts, int n, const void* index, int n_faces, float* sdist, int* visits,
                                  void* stream);

/* ---- closest face of a triangle mesh and the metrics between two meshes (csrc/mesh_closest.hip, csrc/mesh_index.hip;
 * multiply_amd/metrics.py).  The reference has no such code: its evaluation protocol is restated, see DESIGN 6g.  Per point:
 * d2 [n] = the smallest squared distance to a face, face [n] (optional) = the face attaining it, q [n][3] (optional) = the
 * closest point on that face.  Selection: the lexicographic minimum of (d2, face id); a face of zero area ((b-a) x (c-a) == 0)
 * gives NaN and is never selected.  A point with a non-finite coordinate, or a mesh without a face of non-zero area, gives
 * face -1, d2 +inf, q NaN.  Both forms evaluate a face with the same contraction-free arithmetic and return the same bits.
 * Status -1 without a launch: a NULL required argument, n < 0, n_faces <= 0; 0 without a launch: n == 0.  No atomics:
 * bit-identical from call to call.
 *   mp_mesh_closest          : brute force over face_verts [F][3][3]
 *   mp_mesh_index_closest    : through the index of mp_mesh_index_build (layout unchanged); order [n_faces] = the permutation
 *                              given to that build (sorted slot s is face order[s]; the tie rule is on these ids), NULL = the
 *                              sorted slots are reported; visits (optional) as in mp_mesh_index_signed_distance
 *   mp_mesh_index_point_keys : keys [n] = the Hilbert-curve key of each point in the box of the index (points outside fall
 *                              into the border cells): queries sorted by it keep the lanes of a wave on neighbouring walks
 *   mp_mesh_metric_reduce    : d2 [n], face [n] of such a query, normals [n][3] = the samples' own unit normals, face_normals
 *                              [n_faces][3] of the queried mesh (mp_fit_area_cdf), thresholds [n_thresholds <= 8] -> out
 *                              [7 + n_thresholds] DOUBLES: mean sqrt(d2), mean d2, max sqrt(d2), mean n.n', mean |n.n'|, the
 *                              number of samples counted, the number left out (face outside 0 .. n_faces - 1), then per
 *                              threshold the count of sqrt(d2) < threshold.  An empty set's means and max are 0; n == 0
 *                              launches and writes that.  One workgroup, sums in double in a fixed order. */
int mp_mesh_closest(const float* pts, int n, const float* face_verts, int n_faces, float* d2, int* face, float* q, void* stream);
int mp_mesh_index_closest(const float* pts, int n, const void* index, int n_faces, const long long* order, float* d2, int* face,
                          float* q, int* visits, void* stream);
int mp_mesh_index_point_keys(const float* pts, int n, const void* index, int* keys, void* stream);
int mp_mesh_metric_reduce(const float* d2, const int* face, const float* normals, const float* face_normals, int n, int n_faces,
                          const float* thresholds, int n_thresholds, double* out, void* stream);

/* ---- general deformer queries (deformer.py:19-50, 72-88) for K <= 8 nearest vertices; the render / training path uses
 * the fused K = 1 kernels above.  weights [n][24] = sum_k conf_k skin_w[idx_k], conf = exp(-min(d^2,4)) normalised;
 * outlier (optional) = sqrt(min(d_0^2, 4)) > 0.1.  mp_skinning: x' = (sum_j w_j tfs_j) x, or its inverse. */
int mp_query_weights(const float* pts, int n, const float* verts, int n_verts, const float* skin_w, int K, float* weights,
                     unsigned char* outlier, void* stream);
int mp_skinning(const float* pts, const float* weights, int n, const float* tfs, int inverse, float* out, void* stream);

/* ---- input producer (code/lib/datasets/Hi4D.py:8-20 bilinear_interpolation, :59-88 weighted_sampling) --------------
 * Sub-pixel samples of a frame that is RESIDENT in device memory: img [H][W][3] bytes (RGB), mask [H][W] bytes (the sum of
 * the per-person masks, Hi4D.py:236-245), extra [H][W][n_extra] fp32 (optional, e.g. the SAM mask), pos [n][2] doubles
 * (row, col) as the reference draws them (row < H-1, col < W-1).  Outputs (each optional): rgb [n][3] = interpolated
 * img/255, uv [n][2] = (col, row), mask_out [n], extra_out [n][n_extra]; double arithmetic, rounded once to fp32. */
int mp_sample_pixels(const unsigned char* img, const unsigned char* mask, const float* extra, int n_extra,
                     const double* pos, int n, int H, int W, float* rgb, float* uv, float* mask_out, float* extra_out,
                     void* stream);

/* ---- canonical-mesh extraction (code/lib/libmise/mise.pyx: MISE.__cinit__ :33-78, update :80-97, query :99-120,
 * to_dense :122-154, subdivide_voxels :172-222; driver code/lib/utils/mesh.py:78-131) on a DENSE lattice:
 * resolution R = res0 << depth, n = R + 1 points per axis.  state [n^3] bytes (0 no grid point, 1 unknown, 2 known),
 * val [n^3] fp32, vox / pos / neg [sum_l (res0<<l)^3, l = 0..depth] bytes (voxel tree: 0 absent, 1 leaf, 2 split; and
 * the "touches a value >= / <= threshold" flags, which the caller zeroes before every mp_mise_refine).
 *   mp_mise_init    : level-0 voxels are leaves, their corners are unknown grid points
 *   mp_mise_collect : packs the unknown grid points (x, y, z ints, unspecified order) -> out_xyz, *count (device int,
 *                     zeroed by the caller; may exceed max_out, then only max_out were written)
 *   mp_mise_scatter : stores the values of `count` queried points and marks them known
 *   mp_mise_refine  : one update step: mark leaves from ALL known points, split the active ones (*n_split += splits)
 *   mp_mise_fill    : to_dense: holes inherit the previous value along x, then y, then z
 * Marching cubes over the dense values (skimage.measure.marching_cubes in the reference, third party): tri_table
 * [256][16] ints (edge triples, -1 terminated; corner / edge numbering of csrc/mise.hip), case bit k = corner k below
 * `level`; mp_mc_count -> triangles per cube [(n-1)^3]; mp_mc_emit with exclusive-scan offsets -> verts [3T][3] in
 * lattice units and edge_id [3T] (equal ids = same mesh vertex). */
int mp_mise_init(int res0, int depth, unsigned char* state, unsigned char* vox, void* stream);
int mp_mise_collect(int n, const unsigned char* state, int* count, int max_out, int* out_xyz, void* stream);
int mp_mise_scatter(int n, const int* xyz, const float* values, int count, unsigned char* state, float* val, void* stream);
int mp_mise_refine(int res0, int depth, float threshold, unsigned char* state, const float* val, unsigned char* vox,
                   unsigned char* pos, unsigned char* neg, int* n_split, void* stream);
int mp_mise_fill(int n, unsigned char* state, float* val, void* stream);
int mp_mc_count(const float* val, int n, float level, const int* tri_table, int* counts, void* stream);
int mp_mc_emit(const float* val, int n, float level, const int* tri_table, const long long* offsets, float* verts,
               long long* edge_id, void* stream);

/* ---- per-person mesh z-buffer (code/lib/model/render.py:64-66, 134-157 render_multiple_depth_map over pytorch3d's
 * MeshRasterizer with blur_radius 0; callers multiply_model.py:396, :634, :875).  verts [n_verts][3] world space, faces
 * [n_faces][3] ints; cam_host = 16 floats IN HOST MEMORY: R row-major (OpenCV world -> camera), T, fx, fy, cx, cy; a pixel
 * (row, col) is sampled at (col + 0.5, row + 0.5); faces with a vertex nearer than z_clip are dropped.  keys [H*W] and big
 * [n_faces + 1] are scratch.  zbuf [H][W] = camera-space depth of the nearest covering face (-1: none), pix_to_face [H][W]
 * (optional, -1: none), bary [H][W][3] (optional) perspective-correct barycentrics of the winner.  pytorch3d is third
 * party and unpinned: restated, see csrc/raster.hip. */
int mp_raster_zbuf(const float* verts, int n_verts, const int* faces, int n_faces, const float* cam_host, float z_clip,
                   int H, int W, unsigned long long* keys, int* big, float* zbuf, int* pix_to_face, float* bary,
                   void* stream);

/* ---- soft silhouette render (code/lib/model/render.py:79-105, 121-133 softrender_multiple_meshes: pytorch3d's blurred
 * MeshRasterizer + SoftPhongShader under white ambient light = softmax_rgb_blend of the interpolated vertex colours; consumer
 * multiply_model.py:636-637, :721).  Two calls, because the length of the tile lists is only known after the count:
 *   mp_raster_soft_bins  faces -> 8 x 8-pixel tiles: tile_n [T] scratch (T = ceil(H/8) ceil(W/8)), offsets [T + 1] exclusive
 *                        offsets of the tile lists, offsets[T] = total entries (-1: more than INT_MAX)
 *   mp_raster_soft       tile_n / offsets as mp_raster_soft_bins left them for the SAME mesh, camera, image size and
 *                        blur_radius (tile_n all zero again: it counts the list fill); list [offsets[T]] scratch, colors
 *                        [n_verts][3]; image [H][W][4] = RGB over the background + the
 *                        silhouette 1 - prod(1 - prob); sel [H][W][faces_per_pixel] (optional): the selected faces of every
 *                        pixel in no particular order, -1 padded.  faces_per_pixel <= 100.  cam_host / background_host
 *                        (3 floats) IN HOST MEMORY; camera and pixel conventions of mp_raster_zbuf; distances are pytorch3d
 *                        NDC units (the shorter image side spans [-1, 1]), blur_radius a SQUARED distance.
 * pytorch3d is third party and unpinned: restated, see csrc/raster.hip. */
int mp_raster_soft_bins(const float* verts, int n_verts, const int* faces, int n_faces, const float* cam_host, float z_clip,
                        int H, int W, float blur_radius, int* tile_n, int* offsets, void* stream);
int mp_raster_soft(const float* verts, int n_verts, const int* faces, int n_faces, const float* colors, const float* cam_host,
                   float z_clip, int H, int W, float sigma, float gamma, float blur_radius, int faces_per_pixel, float znear,
                   float zfar, const float* background_host, int* tile_n, const int* offsets, int* list, float* image, int* sel,
                   void* stream);

/* ---- fitting an SDF network to a closed triangle mesh (multiply_amd/smpl_init.py; the reference only LOADS such a fit,
 * multiply.py:101-108, its producer is not in its tree): the training points of one iteration and the IGR-style objective
 * (Gropp et al. 2020) with its adjoints.  Randomness comes in as explicit arrays (uniforms in [0,1), standard normals).
 *   mp_fit_area_cdf : face_verts [F][3][3] -> area [F], normal [F][3] (unit, (b-a) x (c-a)), cdf [F] = inclusive cumulative
 *                     area / total (sums in double, fixed order, one workgroup).  A face whose cross product is shorter than
 *                     1e-12 is degenerate: area 0, normal 0, and the search below never selects it.
 *   mp_fit_sample   : surface point i < n_s from u_surf [n_s][3]: face = first f with cdf[f] > u0, barycentrics
 *                     (1 - r, r (1 - u2), r u2), r = sqrt(u1) -> surf_pts [n_s][3], surf_nrm [n_s][3], face_id [n_s];
 *                     volume point j < n_near: surface point (j mod n_s) + sigma_local z_near[j]; j >= n_near: uniform in
 *                     box = [lo3, hi3] (device) from u_box [n_v - n_near][3] -> vol_pts [n_v][3].
 *   mp_fit_loss     : points = the n_s surface points, then the n_v volume points.  sdf [n], grad [n][3] of the network,
 *                     normals [n_s][3], dist [n_v] exact signed distances ->
 *                     terms[5] = total, mean_S |f|, mean_S |grad f - n|_2, mean_V |c(f) - c(dist)| (c = clamp to
 *                     [-truncation, truncation] when truncation > 0, identity otherwise), mean_{S+V} (|grad f|_2 - 1)^2;
 *                     total = w_surface t1 + w_normal t2 + w_distance t3 + w_eikonal t4; d_sdf [n], d_grad [n][3] = its
 *                     gradient.  Norms < 1e-12 and |.| at 0 contribute 0; an empty set's mean is 0.  One workgroup, sums in
 *                     a fixed order: bit-identical from call to call. */
int mp_fit_area_cdf(const float* face_verts, int n_faces, float* area, float* normal, float* cdf, void* stream);
int mp_fit_sample(const float* face_verts, const float* normal, const float* cdf, int n_faces, const float* u_surf, int n_s,
                  const float* z_near, int n_near, float sigma_local, const float* u_box, const float* box, int n_v,
                  float* surf_pts, float* surf_nrm, int* face_id, float* vol_pts, void* stream);
int mp_fit_loss(const float* sdf, const float* grad, const float* normals, const float* dist, int n_s, int n_v,
                float w_surface, float w_normal, float w_distance, float w_eikonal, float truncation, float* terms,
                float* d_sdf, float* d_grad, void* stream);

/* ---- mesh-free interpenetration term on the persons' SDF fields (csrc/penetration.hip; multiply_amd/train.py Interpenetration;
 * the reference's mesh term: multiply_model.py:521-551).  Person p's n probe points (posed SMPL vertices) are warped into
 * partner q's canonical space and penalised by q's signed distance where it is negative.  Every call covers ALL ordered pairs
 * (p, q), p != q, of n_person persons (2 .. 8, the compositing limit); pair index p * n_person + q.  Per-person inputs are device
 * arrays of n_person device pointers; per-pair arrays are [n_person^2][n] rows.  Diagonal pairs are never read or written.
 * Status -1 without a launch: n < 0, n_person outside 2 .. 8, a NULL argument; 0 without a launch: n == 0.  No atomics anywhere:
 * every result is bit-identical from call to call.
 *   mp_pen_probe       : pts[p] [n][3]; vsorted[q] / cbound[q] (mp_knn_build) and blend_table[q] (mp_blend_table) of q's POSED
 *                        vertices.  Exact nearest vertex of q within the outlier radius (the capped search and the rule of
 *                        mp_warp_inverse in eval mode: outlier = sqrtf(fminf(d^2, 4)) > 0.1f, ties -> lowest vertex id) ->
 *                        probed [pair][n] (1 = not an outlier; written for every point), and for the probed points only
 *                        nn [pair][n] (the vertex) and xc [pair][n][3] = I_nn (x - c_nn); list [pair][0 .. count[pair]) = the
 *                        probed point ids in ASCENDING order, count [pair] on the device.
 *   mp_pen_loss        : sdf[pair] = q's signed distance at the list's entries ([count[pair]] floats; NULL allowed where the
 *                        count is 0) -> loss [pair] = sum of s^2 over {s < 0} (summed in double in a fixed order), active [pair]
 *                        = how many, seed[pair] [count[pair]] = 2 s [s < 0]; loss and active of the diagonal are written as 0.
 *                        n = the row length count[] is clamped to.
 *   mp_pen_scatter_bwd : dverts[p] [n_verts][3] += sum over q (ascending) and over the entries e (ascending) of pair (p, q) whose
 *                        point was drawn from vertex v (pen_idx[p][list[pair][e]] == v) of I_nn^T dxc[pair][e]; I_nn from
 *                        blend_table[q] by nn.  One thread per vertex; the draw may repeat a vertex. */
int mp_pen_probe(const float* const* pts, const float* const* vsorted, const float* const* cbound,
                 const float* const* blend_table, int n_person, int n, unsigned char* probed, int* nn, float* xc, int* list,
                 int* count, void* stream);
int mp_pen_loss(const float* const* sdf, const int* count, int n_person, int n, float* loss, int* active, float* const* seed,
                void* stream);
int mp_pen_scatter_bwd(const int* const* pen_idx, const int* list, const int* count, const int* nn,
                       const float* const* blend_table, const float* const* dxc, int n_person, int n, int n_verts,
                       float* const* dverts, void* stream);

/* ---- image-space metrics (csrc/image_metrics.hip; multiply_amd/image_metrics.py, whose docstring holds the definitions; the
 * reference has get_psnr, code/lib/utils/rend_util.py:10-18, and otherwise writes PNGs for an outside script to score).
 * Images a, b [N][H][W][C] fp32, C = 1 or 3, values in [0, data_range]; mask [N][H][W] bytes (non-zero = inside) or NULL = every
 * pixel.  A VALUE is one channel of one pixel.  Both calls write out [N][5] doubles per frame:
 *   out[n] = { sum, number counted, sum over the mask, number counted in the mask, number left out }
 * through per-workgroup partials in `work` (mp_image_work_bytes(N, H, W, C) bytes, 8-byte aligned; -1 for a shape neither call
 * takes) that a finishing pass adds in a fixed order: no atomics, bit-identical from call to call.
 *   mp_image_sqerr : sum of (a - b)^2 in double over the values where a and b are both finite; the others are left out.
 *                    H * W * C < 2^31.
 *   mp_image_ssim  : SSIM (Wang et al. 2004): 11 x 11 Gaussian window, sigma 1.5 (taps formed in double, normalised to sum 1),
 *                    K1 = 0.01, K2 = 0.03, population moments, per channel, only where the whole window lies inside the image:
 *                    the map is [N][H-10][W-10][C].  sum = the sum of the map; a window that holds a non-finite value of a or b
 *                    is left out (map value NaN); a window belongs to the mask when its CENTRE pixel does.  map: the map itself,
 *                    rounded once to fp32, or NULL.  Window sums, moments and the SSIM expression are in double, taken about a
 *                    per-tile pivot so that flat images lose nothing to cancellation; the expression is symmetric in a and b
 *                    (swapping them returns the same bits).  One workgroup per MP_SSIM_TILE x MP_SSIM_TILE tile of the map.
 * Status -1 without a launch: N < 0, C not 1 or 3, a NULL a / b / work / out with N > 0, a grid beyond 2^31 - 1 workgroups;
 * mp_image_ssim also H < 11, W < 11, data_range not a positive finite number; mp_image_sqerr H < 1 or W < 1.  N == 0: returns 0,
 * nothing is read or written. */
#define MP_SSIM_TILE 32
int mp_image_work_bytes(int N, int H, int W, int C);
int mp_image_ssim(const float* a, const float* b, const unsigned char* mask, int N, int H, int W, int C, float data_range,
                  void* work, double* out, float* map, void* stream);
int mp_image_sqerr(const float* a, const float* b, const unsigned char* mask, int N, int H, int W, int C, void* work,
                   double* out, void* stream);

/* ---- pose metrics (multiply_amd/pose_metrics.py, csrc/pose_metrics.hip): MPJPE / MVE and the contact distance.
 *   mp_pose_errors      : M items of n points, pred [M][n][3] against gt [M][n][3], optional roots pred_root / gt_root [M][3]
 *                         (both or neither) -> out [M][4] DOUBLES per item:
 *                           out[0] mean |p_i - x_i|                                  (plain)
 *                           out[1] mean |(p_i - pred_root) - (x_i - gt_root)|        (root-aligned; NaN without roots)
 *                           out[2] mean |s R p_i + t - x_i|, (s, R, t) the least-squares similarity transform with det R = +1
 *                                  (Umeyama 1991): H = sum (p_i - mean p)(x_i - mean x)^T = U S V^T, D = diag(1, 1, sign det(V U^T)),
 *                                  R = V D U^T, s = tr(S D) / sum |p_i - mean p|^2, t = mean x - s R mean p; exactly 0 when the
 *                                  two sets are equal (the identity attains the minimum)
 *                           out[3] 0, or why the item is left out: 1 = a non-finite coordinate (points or roots): all three
 *                                  values NaN; 2 = the predicted points all coincide (sum |p_i - mean p|^2 is exactly 0; tested
 *                                  point against point, a sum about a rounded mean need not be 0): out[2] alone is NaN.
 *                         One workgroup per item, three passes over its points (means and the first two sums; H about the means;
 *                         the residual), every sum in double on the fp32 inputs in a fixed order, the 3 x 3 SVD in double by
 *                         one-sided Jacobi rotations.  Status -1 without a launch: M < 0, n < 1, a NULL pred / gt / out with M > 0,
 *                         exactly one root; M == 0 returns 0.
 *   mp_contact_distance : bodies verts [F][P][V][3], faces [n_faces][3], m correspondences SORTED BY FRAME: corr [m][5] = frame,
 *                         person a, vertex of a, person b, face of b; bary [m][3]; frame_start [F + 1] = the first correspondence of
 *                         each frame (frame_start[F] = m).  Distance of one: | v[f, a, vertex] - sum_k bary_k v[f, b, faces[face][k]] |
 *                         in double; an id out of range (or a frame other than the slot's) gives NaN.  out [2 + 2 F] DOUBLES =
 *                         overall mean (NaN for m = 0), m, then the per-frame means (NaN for a frame without one) and the per-frame
 *                         counts.  One workgroup per frame writes its sum to work [F] doubles, a finishing pass adds those in
 *                         frame order: no atomics, bit-identical from call to call.  Status -1 without a launch: F < 1, P < 1,
 *                         V < 1, n_faces < 1, m < 0, a NULL verts / faces / frame_start / work / out, NULL corr / bary with m > 0. */
int mp_pose_errors(const float* pred, const float* gt, const float* pred_root, const float* gt_root, int M, int n, double* out,
                   void* stream);
int mp_contact_distance(const float* verts, int F, int P, int V, const int* faces, int n_faces, const int* corr, const float* bary,
                        const int* frame_start, int m, double* work, double* out, void* stream);

/* ---- registration of meshes before the mesh metrics (multiply_amd/registration.py, csrc/registration.hip; the reference has no
 * code for it: the paper's protocol aligns the monocular reconstruction, which lives in a normalised frame, to the scans).
 * Point-to-plane ICP for x = s R p + t, rigid (s fixed) or similarity, on closest-surface correspondences.  Everything after the
 * loads is DOUBLE, there are no atomics, partial sums are finished in a fixed order: the same inputs give the same bits.
 *   state [MP_REG_STATE] doubles in device memory, the whole iteration state (indices MP_REG_*):
 *       S scale; R [9] row-major; T [3]; TAU2 the acceptance threshold on |x - q|^2 of the NEXT rows launch (+inf: accept all);
 *       RMS sqrt(sum |x - q|^2 / accepted) of the last step's pairs; ACCEPTED / REJECTED / LEFT_OUT (non-finite) their counts;
 *       ITERS steps taken; FLAG 0 = running, MP_REG_CONVERGED, MP_REG_DEGENERATE; STEP the last step size; C [3] the fixed origin
 *       the rows are formed about; BOX_LO / BOX_HI [3] the target's bounding box; RMS_PLANE sqrt(sum r^2 / accepted).
 *       The host writes S, R, T, TAU2, C, BOX_* (C = the box's centre) and zeroes the rest; the kernels do the rest.
 *   slot [MP_REG_SLOT] doubles, one direction's sums: ATA the 28 entries of the upper triangle of A^T A (row-major, i <= j), ATR
 *       the 7 of A^T r, R2 = sum r^2, D2 = sum |x - q|^2, ACCEPTED / REJECTED / LEFT_OUT counts.
 *   mp_reg_apply     : out[i] = s R p[i] + t (inverse = 0) or R^T (p[i] - t) / s (inverse != 0), the transform read from state, in
 *                      double, rounded once to fp32.  out may be p.
 *   mp_reg_rows      : pairs (p[i] in the source frame, q[i] in the target frame) with unit normals: normals [n][3] per pair when
 *                      face == NULL, else normals [n_faces][3] and face [n] ids into it.  normals_in_source != 0: n = R n.  x = s R p
 *                      + t.  A pair with a non-finite value (or a face id outside [0, n_faces)) is LEFT OUT; one with |x - q|^2 >
 *                      TAU2 is REJECTED; every other adds the row a = [(x - c) x n, n, (x - c) . n], residual r = (x - q) . n, to
 *                      the slot's sums.  mask [n] bytes (may be NULL) receives 0 accepted / 1 rejected / 2 left out.  Workgroup b
 *                      of G = min(ceil(n / 256), MP_REG_MAX_BLOCKS) takes the pairs b 256 + t + k G 256 (thread t, k = 0, 1, ..),
 *                      lanes are added by the xor butterfly, waves in order, and a finishing launch adds the workgroups' partial
 *                      sums work [MP_REG_MAX_BLOCKS][MP_REG_SLOT] in ascending order into slot.  n == 0 writes a zero slot.
 *   mp_reg_step      : ONE workgroup adds slots [n_slots][MP_REG_SLOT] in ascending order, solves the 6 x 6 (similarity == 0) or
 *                      7 x 7 normal equations A^T A delta = -A^T r by Cholesky, composes R <- exp([omega]x) R (Rodrigues), s <- s
 *                      exp(sigma), t <- c + exp(sigma) exp([omega]x) (t - c) + v, and writes RMS, the counts, TAU2 = (reject rms)^2
 *                      (+inf for reject == 0), STEP = the largest displacement of the 8 corners of the box between the old and the
 *                      new transform, and FLAG = MP_REG_CONVERGED when STEP <= tol |BOX_HI - BOX_LO|.  Fewer than 7 accepted pairs
 *                      or a pivot not above 2^-40 of its diagonal entry: FLAG = MP_REG_DEGENERATE, the transform stays.  (The
 *                      routine is csrc/reg_solve.hpp, __host__ __device__.)
 *   Once FLAG != 0 both of the above return without writing anything: a fixed sequence of launches needs no host synchronisation
 *   to stop.
 *   mp_reg_fit_pairs : the closed form (Umeyama 1991) for weighted pairs: means p_, q_ (pass 1), H = sum w (p - p_)(q - q_)^T and
 *                      sum w |p - p_|^2 about them (pass 2), R by the Procrustes routine of csrc/procrustes.hpp, s = tr(S D) / sum
 *                      w |p - p_|^2 (1 when similarity == 0), t = q_ - s R p_.  w == NULL: all 1.  A pair with a non-finite value or
 *                      a weight that is not > 0 is left out.  out [16] doubles = s, R [9], t [3], sum w, pairs left out, status (0;
 *                      1: sum w == 0; 2: the p coincide, s = 1).  One workgroup, the order of k_pose_errors.
 * Status -1 without a launch: a negative size, a NULL required pointer (p / q / normals / out may be NULL only with n == 0),
 * n_slots < 1, n_faces < 1 with a face list, reject < 0 or tol < 0 (or not a number). */
#define MP_REG_STATE 32
#define MP_REG_SLOT 40
#define MP_REG_MAX_BLOCKS 256
enum { MP_REG_S = 0, MP_REG_R = 1, MP_REG_T = 10, MP_REG_TAU2 = 13, MP_REG_RMS = 14, MP_REG_ACCEPTED = 15, MP_REG_REJECTED = 16,
       MP_REG_LEFT_OUT = 17, MP_REG_ITERS = 18, MP_REG_FLAG = 19, MP_REG_STEP = 20, MP_REG_C = 21, MP_REG_BOX_LO = 24,
       MP_REG_BOX_HI = 27, MP_REG_RMS_PLANE = 30 };
enum { MP_REG_SLOT_ATA = 0, MP_REG_SLOT_ATR = 28, MP_REG_SLOT_R2 = 35, MP_REG_SLOT_D2 = 36, MP_REG_SLOT_ACCEPTED = 37,
       MP_REG_SLOT_REJECTED = 38, MP_REG_SLOT_LEFT_OUT = 39 };
enum { MP_REG_CONVERGED = 1, MP_REG_DEGENERATE = 2 };
int mp_reg_apply(const float* p, int n, const double* state, int inverse, float* out, void* stream);
int mp_reg_rows(const float* p, const float* q, const float* normals, const int* face, int n_faces, int normals_in_source, int n,
                const double* state, double* work, double* slot, unsigned char* mask, void* stream);
int mp_reg_step(const double* slots, int n_slots, int similarity, double reject, double tol, double* state, void* stream);
int mp_reg_fit_pairs(const float* p, const float* q, const float* w, int n, int similarity, double* out, void* stream);

/* ---- refining SMPL fits to 2D keypoints (multiply_amd/keypoint_fit.py, csrc/keypoint_fit.hip; the reference's `refine` mode,
 * preprocessing/preprocessing_multiple_trace.py:360-527 with preprocessing/loss.py).  One row = one person in one frame; its free
 * parameters are params [MP_KP_PARAMS] = transl 3, thetas 72, betas 10 (scale 1, absolute transforms).  One workgroup per row.
 *   body      SMPL forward as in csrc/smpl.hip (Rodrigues with angle = |theta + 1e-8|, rest joints J = j_template + j_shapedirs betas,
 *             the chain), and ONLY for the S support vertices v_posed = sv_template + s_shapedirs betas + s_posedirs^T pf, skinned
 *             with s_weights, plus transl.  The "support pack" of table set t: j_template [24][3], j_shapedirs [24][3][10],
 *             sv_template [S][3], s_shapedirs [S][3][10], s_posedirs [207][3S], s_weights [S][24]; n_tables sets lie one after the
 *             other in each array and row_table [N] (NULL: all 0) names a row's set.  parents [24] is shared.
 *   map       keypoint k = sum_m map_w[m] src[map_idx[m]], m in [map_ptr[k], map_ptr[k+1]), src = [24 posed joints ; S support
 *             vertices]; tmap_* is the same matrix by source (tmap_ptr [24 + S + 1], tmap_k / tmap_w [nnz]): the adjoint gathers,
 *             no atomics.  Caps: K <= MP_KP_MAX_K, S <= MP_KP_MAX_S (the row's state lives in 38 KB of LDS), 1 <= K, 0 <= S.
 *   camera    [N][16] = fx, fy, cx, cy, E [3][4]:  x_c = E [x; 1], u = fx x_c / z_c + cx, v = fy y_c / z_c + cy.
 *   loss      terms [3] = { L2d = sum_k c_k sum_{u,v} rho^2 r^2 / (r^2 + rho^2), r = target - projected;
 *                           Lt  = w_p mean_{24x6}((rot6D - rot6D(prev thetas))^2) + mean_3((transl - prev transl)^2);
 *                           w_2d L2d + w_t Lt }
 *             targets [N][K][2], c [N][K] (the host folds confidence, joint weight and 1 / (2 K_set) into c), prev [N][75] = transl,
 *             thetas of the temporal target, held constant (NULL: Lt = 0).  rot6D = the first two columns of a joint's rotation.
 *             A keypoint with z_c <= 0 (or not a number) contributes nothing, its projection is written as 0, and flags [n] = 1.
 *   mp_kp_objective : terms [N][3], grad [N][MP_KP_PARAMS] (of the weighted total), proj [N][K][2], flags [N] ints; terms, grad and
 *                     proj may be NULL.
 *   mp_kp_fit       : iters steps of torch.optim.Adam (bias correction, eps added to the denominator, lr_t / lr_p / lr_b for
 *                     transl / thetas / betas) in ONE launch; parameters, moments and the chain never leave the chip.  out
 *                     [N][MP_KP_PARAMS]; history [N][iters][3] (may be NULL) = the terms evaluated before each step; flags [N] = 1
 *                     if any step met z_c <= 0.  iters = 0 copies params.
 * fp32, fixed-order reductions: the same inputs give the same bits, and a row has the same bits alone and inside any batch.
 * Status -1 without a launch: a NULL required pointer, N < 0, iters < 0, n_tables < 1; -2: K or S outside the caps.  N == 0: 0. */
#define MP_KP_PARAMS 85
#define MP_KP_MAX_K 64
#define MP_KP_MAX_S 256
int mp_kp_objective(const int* parents, const float* j_template, const float* j_shapedirs, const float* sv_template,
                    const float* s_shapedirs, const float* s_posedirs, const float* s_weights, int n_tables, const int* row_table,
                    const int* map_ptr, const int* map_idx, const float* map_w, const int* tmap_ptr, const int* tmap_k,
                    const float* tmap_w, int S, int K, const float* params, const float* prev, const float* targets,
                    const float* c, const float* camera, int N, float rho, float w_2d, float w_t, float w_p, float* terms,
                    float* grad, float* proj, int* flags, void* stream);
int mp_kp_fit(const int* parents, const float* j_template, const float* j_shapedirs, const float* sv_template,
              const float* s_shapedirs, const float* s_posedirs, const float* s_weights, int n_tables, const int* row_table,
              const int* map_ptr, const int* map_idx, const float* map_w, const int* tmap_ptr, const int* tmap_k,
              const float* tmap_w, int S, int K, const float* params, const float* prev, const float* targets, const float* c,
              const float* camera, int N, float rho, float w_2d, float w_t, float w_p, int iters, float lr_t, float lr_p,
              float lr_b, float beta1, float beta2, float eps, float* out, float* history, int* flags, void* stream);

/* ---- building a scene folder from refined fits (multiply_amd/scene_build.py, csrc/raster.hip + csrc/scene.hip; the reference's
 * `final` mode, preprocessing/preprocessing_multiple_trace.py:529-599, which rasterises with pytorch3d and dilates with cv2 on the
 * host, one body at a time).  Masks are [N][H][W] bytes.
 *   mp_raster_mask_batch : coverage of N meshes verts [N][n_verts][3] that share faces [n_faces][3] and ONE camera (cam_host,
 *                          z_clip, the pixel convention: mp_raster_zbuf's): mask[n][r][c] = 255 where mp_raster_zbuf of mesh n
 *                          alone gives zbuf >= 0 (the same projection, box and coverage arithmetic), 0 elsewhere.  big
 *                          [1 + N n_faces] ints is scratch.  Two launches whatever N is; a mesh's mask has the same bytes alone
 *                          and at any position of any batch.  Status -1 without a launch: N, n_verts or n_faces < 0, H or W < 1,
 *                          a NULL cam_host, with N > 0 a NULL mask / big (verts / faces with n_faces > 0), N n_faces >= 2^31 - 1;
 *                          N == 0 returns 0 and touches nothing.
 *   mp_mask_dilate       : out[n][r][c] = 255 if in[n][r + dr][c + dc] != 0 for some dr in [-ay, kh - 1 - ay], dc in [-ax, kw - 1 -
 *                          ax] inside the image, else 0 (cv2.dilate with a kh x kw box of ones and anchor (ax, ay); its default
 *                          anchor is (kw / 2, kh / 2)).  in and out must not overlap.  Status -2 without a launch: kh or kw outside
 *                          1 .. MP_DILATE_MAX_K, ay outside [0, kh), ax outside [0, kw); -1: N < 0, H or W < 1, with N > 0 a NULL
 *                          or aliased pointer, N > 65535; N == 0 returns 0.
 *   mp_mask_stats        : stats [N][7] 64-bit integers of the nonzero pixels = { count, min row, max row, min col, max col,
 *                          sum of rows, sum of cols }; an empty mask gives { 0, H, -1, W, -1, 0, 0 }.  Integer arithmetic: exact
 *                          whatever the order.  Status -1 without a launch: N < 0, H or W < 1, with N > 0 a NULL pointer, N > 65535.
 *   mp_verts_bounds      : verts [F][n][3].  shift == NULL: out [F][6] = min x, y, z, max x, y, z of frame f (the values of
 *                          torch.amin / amax);  shift [F][3]: out [F] = max_i |v_i + shift_f| in fp32.  One workgroup per frame,
 *                          no atomics.  Finite inputs.  Status -1 without a launch: F < 0, n < 1, with F > 0 a NULL verts / out;
 *                          F == 0 returns 0. */
#define MP_DILATE_MAX_K 64
int mp_raster_mask_batch(const float* verts, int N, int n_verts, const int* faces, int n_faces, const float* cam_host, float z_clip,
                         int H, int W, int* big, unsigned char* mask, void* stream);
int mp_mask_dilate(const unsigned char* in, int N, int H, int W, int kh, int kw, int ay, int ax, unsigned char* out, void* stream);
int mp_mask_stats(const unsigned char* mask, int N, int H, int W, long long* stats, void* stream);
int mp_verts_bounds(const float* verts, int F, int n, const float* shift, float* out, void* stream);

/* ---- the optimiser of the training loop (multiply_amd/trainer.py DeviceAdam, csrc/optim.hip; the reference steps two
 * torch.optim.Adam objects from Lightning's loop, multiply_model.py:62-78, 212-225).
 * mp_adam_multi: torch.optim.Adam's single-tensor step (no weight decay, no amsgrad) for every tensor of an optimiser in ONE
 * launch.  descs = DEVICE array of n_desc records; the blocks (256 threads) of all tensors are concatenated in one grid: block0 =
 * first block of a tensor (ascending from 0), n_block >= 1 its number of blocks, total_blocks = their sum; a tensor with more
 * elements than its blocks cover in one pass is strided over.
 *   p, m (exp_avg), v (exp_avg_sq) [n] are updated in place from g [n]:  m = fma(g - m, 1 - beta1, m);  v = fma(v, beta2,
 *   ((1 - beta2) g) g);  p = fma(-lr[group] / (1 - beta1^t), m / (sqrt(v) / sqrt(1 - beta2^t) + eps), p)  with t = *step + 1 and
 *   the two bias corrections computed in double, as torch's python scalars are.
 *   step  : the tensor's own count, ONE device float (torch's state['step']).  The update kernel only reads the counts; a
 *           trailing n_desc-thread launch on the same stream adds 1 to the count of every active tensor, so no block ever sees
 *           t + 1 for t.  (No ping-pong buffers: the counts stay where the state dict has them.)
 *   g == NULL : the record is inactive -- nothing of it is read or written and its count does not advance (torch: p.grad is None).
 *   mode  : MP_ADAM_SCALAR = 4-byte accesses; MP_ADAM_VEC = 16-byte accesses between a scalar head and tail, valid when p, g, m, v
 *           share their address modulo 16; MP_ADAM_VEC_G4 = the same with g read by dwords, valid when p, m, v share it (gradients
 *           are views of a flat buffer at arbitrary float offsets).  The caller sets the mode from the addresses.
 *   lr    : DEVICE floats, one per group;  skip : DEVICE byte or NULL: when *skip != 0 the launch changes nothing, no count advances.
 * No allocation, no synchronisation.  Status -1 without a launch: n_desc or total_blocks < 0, with n_desc > 0 a NULL descs / lr;
 * -2: beta1 / beta2 outside [0, 1) or eps < 0; n_desc == 0 or total_blocks == 0 returns 0 and touches nothing. */
enum { MP_ADAM_SCALAR = 0, MP_ADAM_VEC = 1, MP_ADAM_VEC_G4 = 2 };
typedef struct {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* step;
    long long n;
    int group, block0, n_block, mode;
} MpAdamDesc;
int mp_adam_multi(const MpAdamDesc* descs, int n_desc, int total_blocks, const float* lr, const unsigned char* skip, double beta1,
                  double beta2, double eps, void* stream);

/* ---- shaded mesh overlays: the QC images of preprocessing and testing (multiply_amd/overlay.py, csrc/overlay.hip; the reference
 * draws them one mesh at a time with pytorch3d and cv2.circle, preprocessing_multiple_trace.py:330-342, 496-510 and
 * ait_viewer_vis/vis_mesh_image.py; both are third party and unpinned, so the rule below is the project's own).
 *   mp_mesh_vertex_normals   : N meshes verts [N][V][3] that share faces [n_faces][3]: normals[n][v] = s / max(|s|, 1e-6) with s =
 *                              sum of cross(v1 - v0, v2 - v0) over the faces adj_face[adj_ptr[v] .. adj_ptr[v + 1]) (the faces
 *                              that contain v, ascending, once per occurrence; built on the host once per topology).  One thread
 *                              per vertex, no atomics: a mesh's normals have the same bits alone and at any position of any
 *                              batch; a vertex of no face gives 0.  Status -1 without a launch: N, V or n_faces < 0, with N V > 0
 *                              a NULL verts / adj_ptr / normals (faces / adj_face with n_faces > 0), N V >= 2^31; N V == 0 returns
 *                              0 and touches nothing.
 *   mp_overlay_vertex_colors : colors [N][V][3] from normals [N][V][3].  MP_OVERLAY_NORMAL: (0.5 n + 0.5) with the channels
 *                              reversed (z, y, x);  MP_OVERLAY_SHADE: d = max(n . light, 0) on all three channels;
 *                              MP_OVERLAY_TINT: tint[n][ch] (ambient + (1 - ambient) d), tint [N][3] DEVICE floats.  light =
 *                              (lx, ly, lz) as given (not normalised).  Status -1 without a launch: N or V < 0, with N V > 0 a
 *                              NULL normals / colors (tint in tint mode), N V >= 2^31; -2: an unknown mode; N V == 0 returns 0
 *                              and touches nothing.
 *   mp_overlay_batch         : n_rec meshes into M images [H][W][3] bytes.  recs = DEVICE array of MpOverlayMesh: verts [n_verts][3]
 *                              world space, faces [n_faces][3], colors [n_verts][3] (records may share any of them), image in
 *                              [0, M), face_base = the exclusive prefix sum of n_faces over the table, block0 = that of
 *                              ceil(n_faces / 256); total_faces and total_blocks are the two sums.  cams_host [n_cam][16] HOST
 *                              floats, n_cam = 1 (all images) or M, mp_raster_zbuf's layout and pixel convention; z_clip its.
 *                              Visibility is mp_raster_zbuf's rule with the same projection, box and coverage arithmetic: one
 *                              64-bit atomicMin per covered pixel on keys [M][H][W] with key = depth bits << 32 | (face_base + f),
 *                              so ties go to the earlier record, then the lower face: what mp_raster_zbuf gives on an image's
 *                              meshes joined in record order.  The grid is the records' face blocks concatenated (a block finds
 *                              its record by binary search); faces whose pixel box exceeds 48 centres go through the queue big
 *                              [1 + total_faces] and a second launch; the number of launches does not depend on n_rec.
 *                              The resolve pass (one thread per pixel) recomputes the winner's perspective-correct barycentrics,
 *                              c = b0 c0 + b1 c1 + b2 c2 per channel, the mesh byte m = floor(255 clamp(c, 0, 1)), and with f =
 *                              the byte of frames [M][H][W][3] (frames == NULL: of background_host, 3 HOST bytes):
 *                              out = floor(fmaf(opacity, m - f, f) + 0.5);  an uncovered pixel keeps f.  Keypoints are painted
 *                              last: keypoints [M][K][3] = (x, y, conf), kp_rgb [K][3] bytes: pixel (r, c) takes keypoint k's
 *                              colour when conf > kp_conf, x and y are finite and (c - floor x)^2 + (r - floor y)^2 <=
 *                              kp_radius^2 in integers; the highest such k wins.  owner [M][H][W] (optional) = the winner's
 *                              record or -1.  Scratch: keys, big, cam_dev [n_cam][16] floats (the cameras' device copy).
 *                              Status -1 without a launch: n_rec, total_blocks, total_faces, M or K < 0, H or W < 1, with M > 0
 *                              a NULL cams_host / keys / cam_dev / out (background_host with NULL frames; recs / big with n_rec >
 *                              0; keypoints / kp_rgb with K > 0), M H W >= 2^31;  -2: n_cam not 1 or M, total_faces >= 2^32 - 1,
 *                              opacity outside [0, 1], kp_radius outside [0, 4096];  M == 0 returns 0 and touches nothing.
 *                              n_rec == 0 with M > 0 gives the frames (background) plus the keypoints. */
enum { MP_OVERLAY_NORMAL = 0, MP_OVERLAY_SHADE = 1, MP_OVERLAY_TINT = 2 };
typedef struct {
    const float* verts;
    const int* faces;
    const float* colors;
    int n_verts, n_faces, image, block0;
    unsigned face_base;
    int pad_;
} MpOverlayMesh;
int mp_mesh_vertex_normals(const float* verts, int N, int V, const int* faces, int n_faces, const int* adj_ptr, const int* adj_face,
                           float* normals, void* stream);
int mp_overlay_vertex_colors(const float* normals, int N, int V, int mode, const float* tint, float lx, float ly, float lz,
                             float ambient, float* colors, void* stream);
int mp_overlay_batch(const MpOverlayMesh* recs, int n_rec, int total_blocks, long long total_faces, int M, int H, int W,
                     const float* cams_host, int n_cam, float z_clip, const unsigned char* frames,
                     const unsigned char* background_host, float opacity, const float* keypoints, int K,
                     const unsigned char* kp_rgb, float kp_conf, int kp_radius, unsigned long long* keys, unsigned* big,
                     float* cam_dev, unsigned char* out, int* owner, void* stream);

/* ---- mesh simplification: vertex clustering with quadric-optimal representatives (Lindstrom 2000; multiply_amd/simplify.py,
 * csrc/simplify.hip, csrc/quadric_solve.hpp).  The reference has no counterpart.  The host sorts (torch) between the
 * launches; everything that reads a coordinate is here.  Index arrays that torch's sorts and prefix sums produce are long long.
 *   mp_simplify_keys     : key[v] = i << 42 | j << 21 | k with (i, j, k) = floor((verts[v] - lo) * inv_h) per axis in fp32, one
 *                          subtraction and one multiplication, each rounded to nearest and never contracted; an index is clamped
 *                          to [0, MP_SIMPLIFY_MAX_INDEX] (the host checks the bounding box first, so nothing is).  One thread per
 *                          vertex.
 *   mp_simplify_count    : live[f] = 1 when the keys of face f's three corners are pairwise different, else 0 (the count pass of
 *                          the target-face bisection; needs no cell ids).  A corner outside [0, n_verts) gives 0.
 *   mp_simplify_faces    : cell [n_verts] = each vertex's cell id (rank of its key).  tri[f] = the ids of the corners in the face's
 *                          own order, live[f] as above, key_lo[f] = min << 32 | mid and key_hi[f] = max of the three ids (the
 *                          unordered triple); a face that is not live gets key_lo = 2^63 - 1, key_hi = 2^31 - 1 and sorts last.
 *   mp_simplify_first    : order [n_faces] = the faces sorted by (key_lo, key_hi), stably, so equal triples are in ascending face
 *                          order: keep[order[s]] = live and (s == 0 or the triple of order[s - 1] differs).
 *   mp_simplify_quadrics : per cell c (keys [n_cells] ascending): centre = lo + (ijk + 0.5) h in double.  pair_order
 *                          [pair_start[c] .. pair_start[c + 1]) = the pair indices 3 f + corner whose corner lies in c, ascending
 *                          (a stable sort of tri); each adds n n^T and n (n . (p0 - centre)), n = (p1 - p0) x (p2 - p0), in
 *                          double.  vert_order [vert_start[c] .. vert_start[c + 1]) = the cell's own vertices, ascending: their
 *                          mean relative to the centre.  MP_SIMPLIFY_LANES lanes share a cell: lane l adds entries l, l + LANES,
 *                          ... of each list in order, the lanes are added by the xor butterfly -- a fixed order, no atomics, the
 *                          same bits on every run.  Then quadric_point (quadric_solve.hpp) and pos[c] = (float)(centre + x).
 *   mp_simplify_attr_mean: out[c][k] = (float)(sum of attrs[v][k] over the cell's vertices in vert_order, in double / their number),
 *                          one thread per (c, k).
 *   Status -1 without a launch: a negative size, a NULL array that the sizes make necessary, inv_h / h / lam not positive and
 *   finite, 3 n_faces >= 2^31, n_cells K >= 2^38.  A size of zero returns 0 and touches nothing (no launch with an empty grid). */
#define MP_SIMPLIFY_BITS 21
#define MP_SIMPLIFY_MAX_INDEX ((1 << MP_SIMPLIFY_BITS) - 1)
#define MP_SIMPLIFY_LANES 16
int mp_simplify_keys(const float* verts, int n_verts, float lo_x, float lo_y, float lo_z, float inv_h, long long* key, void* stream);
int mp_simplify_count(const int* faces, int n_faces, const long long* key, int n_verts, unsigned char* live, void* stream);
int mp_simplify_faces(const int* faces, int n_faces, const int* cell, int n_verts, int* tri, long long* key_lo, int* key_hi,
                      unsigned char* live, void* stream);
int mp_simplify_first(const long long* order, int n_faces, const long long* key_lo, const int* key_hi, const unsigned char* live,
                      unsigned char* keep, void* stream);
int mp_simplify_quadrics(const float* verts, int n_verts, const int* faces, int n_faces, const long long* keys, int n_cells,
                         const long long* pair_order, const long long* pair_start, const long long* vert_order,
                         const long long* vert_start, float lo_x, float lo_y, float lo_z, float h, double lam, float* pos,
                         void* stream);
int mp_simplify_attr_mean(const float* attrs, int n_verts, int K, const long long* vert_order, const long long* vert_start,
                          int n_cells, float* out, void* stream);

/* library / device info: returns the gfx arch string compiled in, and checks the current device */
const char* mp_arch(void);
int mp_device_ok(void);

#ifdef __cplusplus
}
#endif
#endif
