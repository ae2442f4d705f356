"""From refined SMPL fits to a scene folder that `datasets.py` trains on: the `final` stage and the numeric half of the `mask` stage
of the reference's preprocessing (preprocessing/preprocessing_multiple_trace.py:157-163, 274-358, 208-234, 529-599) and its
preprocessing/normalize_cameras_trace.py:6-61, over a whole sequence at once on the device.

`build_scene` takes what keypoint_fit.refine_sequence returns (pose, trans, shape per person-frame in camera space) and produces
poses.npy, normalize_trans.npy, mean_shape.npy, gender.npy, cameras.npz, max_human_sphere.npy, cameras_normalize.npz, mask/<p>/*.png
and image/*.png; with overlays=True also the QC images overlay/<p>/*.png and overlay/all/*.png (write_overlays).  Its definitions, in the order they are applied:

  1 mean shape     mean_shape[p] = mean over the frames of shape[:, p] (:590-592); every body below is posed with it (:552-557).
  2 scene space    per person-frame, float64 on the host (transform_smpl_remain_extrinsic, :72-84): with the current extrinsic
                   [Rc | tc] (identity unless `extrinsic` is given), Rt = diag(1, -1, -1) and T_hip = the rest-pose root joint of the
                   shaped template,
                       R_root' = Rt^-1 Rc R_root,   e = Rc (trans + T_hip) + tc - trans - Rt T_hip,   trans' = Rt^-1 trans + Rt^-1 e
                   so that every vertex obeys Rt v' = Rc v + tc; the extrinsic becomes [Rt | 0].
  3 posing         SMPLServer.pose_batch, one call per person, scale 1, absolute transforms.
  4 bounds, shift  shift_f = -(vmax_f + vmin_f) / 2 over all persons' vertices of frame f (normalize='per_frame', the reference's
                   default branch) or shift_0 for every frame ('first_frame', its hi4d branch); normalize_trans = trans' + shift_f;
                   E_f = [Rt | -Rt shift_f]; cam_f = K4 E_f with fx, fy, cx, cy divided by scale_factor (:223-228);
                   max_human_sphere = max_f max_v |v' + shift_f|  (:563-588).
  5 normalisation  camera centres from cam_f (datasets.load_K_Rt_from_P), r = 1.1 max |centre|, replaced by 1.1 max_human_sphere
                   when that is larger; scale_mat = diag(r/3, r/3, r/3, 1) float32, world_mat_f = cam_f
                   (normalize_cameras_trace.py:28-61).
  6 silhouettes    the camera-space vertices Rt (v' + shift_f) - Rt shift_f = Rt v' of all F P bodies through mp_raster_mask_batch at
                   (H // s, W // s) with the divided intrinsics.
  7 dilation       by a dilate x dilate box of ones with cv2's default anchor dilate // 2 (:230, :542): mp_mask_dilate.

Deviations from the reference, all forced by what it delegates to third parties:
  * it rasterises at full size and resizes the mask with cv2.resize (bilinear); here the silhouette is rendered AT the output size:
    the outlines differ by less than a pixel, under a 20-pixel dilation;
  * frames are reduced with PIL.Image.reduce (a box filter), not cv2's bilinear resize; with scale_factor 1 they are re-encoded
    unchanged;
  * estimate_translation is the deterministic weighted least-squares translation, not cv2.solvePnPRansac's (see there).
"""
import ctypes as C
import os

import numpy as np
import torch

from . import hip
from .datasets import load_K_Rt_from_P
from .render import Z_CLIP

RT = np.diag([1.0, -1.0, -1.0])
NORMALIZE_MODES = ("per_frame", "first_frame")
SCENE_SPHERE = 3.0                     # normalize_cameras_trace.py: scene_bounding_sphere
STAT_KEYS = ("count", "bbox", "centre")


# ------------------------------------------------------------------------------------------------ device wrappers
def raster_mask_batch(verts, faces, cam16, H, W, rows_per_call=None, out=None):
    """verts (N, V, 3) device fp32, faces (F, 3), cam16: the 16 host floats of mp_raster_zbuf's camera -> masks (N, H, W) uint8
    0 / 255 (mp_raster_mask_batch).  rows_per_call bounds the meshes of one kernel call (its queue is 4 (1 + rows F) bytes); a
    mesh's bytes do not depend on it."""
    hip.require_device()
    if verts.dim() != 3 or verts.shape[-1] != 3:
        raise ValueError(f"verts: expected (N, V, 3), got {tuple(verts.shape)}")
    if rows_per_call is not None and int(rows_per_call) < 1:
        raise ValueError(f"rows_per_call must be at least 1, got {rows_per_call}")
    v = verts.detach().float().contiguous()
    f = faces.reshape(-1, 3).to(device=v.device, dtype=torch.int32).contiguous()
    N, nf = v.shape[0], f.shape[0]
    mask = torch.empty(N, H, W, dtype=torch.uint8, device=v.device) if out is None else out
    step = max(N, 1) if rows_per_call is None else int(rows_per_call)
    step = max(1, min(step, (2 ** 31 - 2) // max(nf, 1)))
    big = torch.empty(1 + min(step, max(N, 1)) * nf, dtype=torch.int32, device=v.device)
    cam = (C.c_float * 16)(*[float(x) for x in cam16])
    for s in range(0, N, step):
        e = min(N, s + step)
        hip.lib().mp_raster_mask_batch(v[s:e], e - s, v.shape[1], f, nf, C.cast(cam, C.c_void_p), Z_CLIP, H, W, big, mask[s:e],
                                       hip.stream())
    return mask


def mask_dilate(masks, kh, kw=None, ay=None, ax=None):
    """masks (N, H, W) uint8 -> 0 / 255 dilation by a kh x kw box with anchor (ay, ax) (default: cv2's, k // 2)  (mp_mask_dilate)"""
    kw = kh if kw is None else kw
    ay, ax = kh // 2 if ay is None else ay, kw // 2 if ax is None else ax
    m = masks.contiguous()
    out = torch.empty_like(m)
    hip.lib().mp_mask_dilate(m, m.shape[0], m.shape[1], m.shape[2], kh, kw, ay, ax, out, hip.stream())
    return out


def mask_stats(masks):
    """masks (N, H, W) uint8 -> (N, 7) int64: count, min / max row, min / max col, sum of rows, sum of cols  (mp_mask_stats)"""
    m = masks.contiguous()
    st = torch.empty(m.shape[0], 7, dtype=torch.int64, device=m.device)
    hip.lib().mp_mask_stats(m, m.shape[0], m.shape[1], m.shape[2], st, hip.stream())
    return st


def verts_bounds(verts, shift=None):
    """verts (F, n, 3) device fp32.  shift None: (F, 6) = min xyz, max xyz; shift (F, 3): (F,) = max_i |v_i + shift_f|
    (mp_verts_bounds)"""
    v = verts.detach().float().contiguous()
    F = v.shape[0]
    if shift is None:
        out = torch.empty(F, 6, dtype=torch.float32, device=v.device)
    else:
        shift = shift.detach().to(device=v.device, dtype=torch.float32).reshape(F, 3).contiguous()
        out = torch.empty(F, dtype=torch.float32, device=v.device)
    hip.lib().mp_verts_bounds(v, F, v.shape[1], shift, out, hip.stream())
    return out


def stats_dict(st, shape):
    """(N, 7) int64 of mask_stats -> dict of numpy arrays shaped `shape`: count, bbox (.., 4) = min row, max row, min col, max col,
    centre (.., 2) = mean (col, row) of the nonzero pixels (get_mask_center; NaN for an empty mask)"""
    s = st.cpu().numpy().reshape(tuple(shape) + (7,))
    cnt = s[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        centre = np.stack([s[..., 6] / cnt, s[..., 5] / cnt], -1)
    return {"count": cnt.copy(), "bbox": s[..., 1:5].copy(), "centre": np.where(cnt[..., None] > 0, centre, np.nan)}


# ------------------------------------------------------------------------------------------------ host arithmetic (float64)
def rotvec_to_matrix(r):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(r, np.float64)).as_matrix()


def matrix_to_rotvec(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(np.asarray(R, np.float64)).as_rotvec()


def extrinsic_Rt(extrinsic):
    """None / (3, 4) / (4, 4) world-to-camera -> Rc (3, 3), tc (3,) float64"""
    if extrinsic is None:
        return np.eye(3), np.zeros(3)
    E = np.asarray(extrinsic, np.float64)
    if E.shape not in ((3, 4), (4, 4)):
        raise ValueError(f"extrinsic: expected (3, 4) or (4, 4), got {E.shape}")
    return E[:3, :3].copy(), E[:3, 3].copy()


def rest_root_joint(server, betas):
    """T_hip (3,) float64: row 0 of J_regressor (v_template + shapedirs betas) (smplx body_models.py:279-286)"""
    t = server.tables
    j0 = (t.j_regressor[0].double().cpu() @ t.v_template.double().cpu()).numpy()
    return j0 + t.j_shapedirs[0].double().cpu().numpy() @ np.asarray(betas, np.float64)


def to_scene_space(pose, trans, T_hip, extrinsic=None):
    """transform_smpl_remain_extrinsic (:72-84) on arrays: pose (..., 72), trans (..., 3), T_hip (3,) or broadcastable -> pose',
    trans' float64 with  Rt v' = Rc v + tc  for every vertex of the body."""
    Rc, tc = extrinsic_Rt(extrinsic)
    pose = np.array(pose, np.float64)
    trans = np.asarray(trans, np.float64)
    T_hip = np.broadcast_to(np.asarray(T_hip, np.float64), trans.shape)
    lead = pose.shape[:-1]
    R_root = rotvec_to_matrix(pose[..., :3].reshape(-1, 3))
    pose[..., :3] = matrix_to_rotvec(np.einsum("ij,jk,nkl->nil", RT.T, Rc, R_root)).reshape(lead + (3,))
    e = (trans + T_hip) @ Rc.T + tc - trans - T_hip @ RT.T
    return pose, trans @ RT + e @ RT              # Rt^-1 = Rt^T = Rt; (Rt^-1 x)^T = x^T Rt


def intrinsics4(intrinsics, scale_factor=1):
    """(3, 3) / (4, 4) -> 4 x 4 float64 with fx, fy, cx, cy divided by scale_factor (:223-228)"""
    K = np.eye(4)
    K[:3, :3] = np.asarray(intrinsics, np.float64)[:3, :3]
    for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)):
        K[i, j] /= scale_factor
    return K


def shifts_from_bounds(bounds, normalize="per_frame"):
    """bounds (F, 6) = min xyz, max xyz of every frame's vertices -> shift (F, 3) float64 = -(vmax + vmin) / 2 per frame, or
    frame 0's for every frame ('first_frame')  (:563-573)"""
    if normalize not in NORMALIZE_MODES:
        raise ValueError(f"normalize must be one of {NORMALIZE_MODES}, got {normalize!r}")
    b = np.asarray(bounds, np.float64)
    shift = -(b[:, 3:] + b[:, :3]) / 2.0
    return np.tile(shift[:1], (b.shape[0], 1)) if normalize == "first_frame" else shift


def frame_cameras(K4, shift):
    """shift (F, 3) -> cam (F, 4, 4): K4 [Rt | -Rt shift_f]  (:583-588)"""
    F = shift.shape[0]
    E = np.tile(np.eye(4), (F, 1, 1))
    E[:, :3, :3] = RT
    E[:, :3, 3] = -(shift @ RT.T)
    return K4[None] @ E


def normalize_cameras(cams, max_human_sphere):
    """normalize_cameras_trace.py:28-61.  cams (F, 4, 4) -> dict of scale_mat_%d (float32, shared) and world_mat_%d, and the
    radius r."""
    centres = np.stack([load_K_Rt_from_P(c[:3, :4])[1][:3, 3].astype(np.float64) for c in cams])
    r = np.linalg.norm(centres, axis=1).max() * 1.1
    if max_human_sphere * 1.1 > r:
        r = max_human_sphere * 1.1
    norm = np.eye(4).astype(np.float32)
    norm[0, 0] = norm[1, 1] = norm[2, 2] = r / SCENE_SPHERE
    out = {}
    for i, c in enumerate(cams):
        out["scale_mat_%d" % i] = norm
        out["world_mat_%d" % i] = c.copy()
    return out, float(r)


# ------------------------------------------------------------------------------------------------ the builder
def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def build_scene(servers, refined, intrinsics, img_size, out_dir=None, frames=None, genders=None, normalize="per_frame", dilate=20,
                scale_factor=1, extrinsic=None, rows_per_call=None, overlays=False):
    """servers: one SMPLServer per person, or one for all (as refine_sequence); refined: dict of pose (F, P, 72), trans (F, P, 3),
    shape (F, P, 10) in camera space; intrinsics (3, 3); img_size (H, W) of the frames; frames: F PNG paths or None (no image/);
    genders: P names for gender.npy (default 'neutral', :594).  Returns a dict: poses (F, P, 72), normalize_trans (F, P, 3),
    mean_shape (P, 10), cameras {cam_%d}, cameras_normalize {scale_mat_%d, world_mat_%d}, max_human_sphere, radius, shift (F, 3),
    masks / raw_masks (F, P, H // s, W // s) uint8 device tensors (0 / 255; dilated / as rasterised), mask_stats {'raw', 'dilated'}
    -> {count (F, P), bbox (F, P, 4), centre (F, P, 2)} and img_size.  With out_dir the folder datasets.py reads is written (the
    module docstring has every definition and the deviations from the reference).  The silhouettes are rendered at the OUTPUT size
    (H // s, W // s) with the divided intrinsics, where the reference renders at full size and resizes the mask: less than a pixel
    at the outline, under the dilation.
    overlays (needs out_dir and frames): also writes the QC images overlay/<p>/%04d.png and overlay/all/%04d.png (write_overlays)."""
    hip.require_device()
    if overlays and (out_dir is None or frames is None):
        raise ValueError("overlays are drawn over the written image/ folder: they need out_dir and frames")
    if normalize not in NORMALIZE_MODES:
        raise ValueError(f"normalize must be one of {NORMALIZE_MODES}, got {normalize!r}")
    s = int(scale_factor)
    if s < 1 or s != scale_factor:
        raise ValueError(f"scale_factor: a positive integer, got {scale_factor!r}")
    dilate = int(dilate)
    if dilate < 0 or dilate > 64:
        raise ValueError(f"dilate: 0 .. 64, got {dilate}")
    pose, trans, shape = (np.asarray(_np(refined[k]), np.float64) for k in ("pose", "trans", "shape"))
    if pose.ndim != 3 or pose.shape[2] != 72 or trans.shape != pose.shape[:2] + (3,) or shape.shape != pose.shape[:2] + (10,):
        raise ValueError(f"refined: expected pose (F, P, 72), trans (F, P, 3), shape (F, P, 10), got {pose.shape}, {trans.shape}, "
                         f"{shape.shape}")
    F, P = pose.shape[:2]
    if F < 1 or P < 1:
        raise ValueError("refined: at least one frame and one person")
    servers = list(servers) if isinstance(servers, (list, tuple)) else [servers]
    if len(servers) not in (1, P):
        raise ValueError(f"servers: expected one per person ({P}) or one for all, got {len(servers)}")
    servers = servers * P if len(servers) == 1 else servers
    if any(not np.array_equal(sv.faces, servers[0].faces) for sv in servers[1:]):
        raise ValueError("servers: the persons' bodies must share one face table (one rasteriser call covers them all)")
    genders = ["neutral"] * P if genders is None else list(genders)
    if len(genders) != P:
        raise ValueError(f"genders: expected {P} names, got {len(genders)}")
    if frames is not None and len(frames) != F:
        raise ValueError(f"frames: expected {F} paths, got {len(frames)}")
    H, W = int(img_size[0]) // s, int(img_size[1]) // s
    dev = servers[0].param_canonical.device

    # 1, 2: mean shape, scene space
    mean_shape = shape.mean(0)
    T_hip = np.stack([rest_root_joint(servers[p], mean_shape[p]) for p in range(P)])
    pose_s, trans_s = to_scene_space(pose, trans, T_hip[None], extrinsic)
    # 3: posing
    verts = torch.empty(F, P, servers[0].tables.v_template.shape[0], 3, dtype=torch.float32, device=dev)
    for p in range(P):
        prm = np.concatenate([np.ones((F, 1)), trans_s[:, p], pose_s[:, p], np.tile(mean_shape[p], (F, 1))], 1)
        verts[:, p] = servers[p].pose_batch(torch.from_numpy(prm).float(), absolute=True, want=("verts",),
                                            rows_per_call=rows_per_call)["verts"]
    # 4: bounds and shift
    flat = verts.reshape(F, -1, 3)
    shift = shifts_from_bounds(verts_bounds(flat).double().cpu().numpy(), normalize)
    max_human_sphere = float(verts_bounds(flat, torch.from_numpy(shift)).max())
    normalize_trans = trans_s + shift[:, None, :]
    K4 = intrinsics4(intrinsics, s)
    cams = frame_cameras(K4, shift)
    # 5
    cameras_normalize, radius = normalize_cameras(cams, max_human_sphere)
    # 6, 7: one camera for every body: [Rt | 0] (E_f applied to v' + shift_f)
    cam16 = list(RT.reshape(-1)) + [0.0, 0.0, 0.0, K4[0, 0], K4[1, 1], K4[0, 2], K4[1, 2]]
    faces = torch.from_numpy(np.ascontiguousarray(servers[0].faces)).to(dev)
    raw = raster_mask_batch(verts.reshape(F * P, -1, 3), faces, cam16, H, W, rows_per_call)
    masks = mask_dilate(raw, dilate) if dilate > 1 else raw.clone()
    stats = {"raw": stats_dict(mask_stats(raw), (F, P)), "dilated": stats_dict(mask_stats(masks), (F, P))}
    out = dict(poses=pose_s, normalize_trans=normalize_trans, mean_shape=mean_shape, shift=shift,
               cameras={"cam_%d" % f: cams[f] for f in range(F)}, cameras_normalize=cameras_normalize,
               max_human_sphere=max_human_sphere, radius=radius, masks=masks.reshape(F, P, H, W), raw_masks=raw.reshape(F, P, H, W),
               mask_stats=stats, img_size=(H, W), genders=genders)
    if out_dir is not None:
        write_scene(out_dir, out, frames, s)
        if overlays:
            write_overlays(out_dir, verts, faces, cam16, (H, W), rows_per_call)
    return out


def write_scene(out_dir, scene, frames=None, scale_factor=1):
    """the folder of datasets.py:5-6 (+ cameras.npz and max_human_sphere.npy, :598-599) from build_scene's dict"""
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    F, P = scene["poses"].shape[:2]
    np.save(os.path.join(out_dir, "gender.npy"), np.array(scene["genders"]))
    np.save(os.path.join(out_dir, "poses.npy"), scene["poses"])
    np.save(os.path.join(out_dir, "mean_shape.npy"), scene["mean_shape"])
    np.save(os.path.join(out_dir, "normalize_trans.npy"), scene["normalize_trans"])
    np.savez(os.path.join(out_dir, "cameras.npz"), **scene["cameras"])
    np.save(os.path.join(out_dir, "max_human_sphere.npy"), np.array(scene["max_human_sphere"]))
    np.savez(os.path.join(out_dir, "cameras_normalize.npz"), **scene["cameras_normalize"])
    for p in range(P):
        os.makedirs(os.path.join(out_dir, "mask", "%d" % p), exist_ok=True)
    for f in range(F):
        m = scene["masks"][f].cpu().numpy()                  # a frame at a time: the host never holds the whole sequence
        for p in range(P):
            Image.fromarray(m[p], mode="L").save(os.path.join(out_dir, "mask", "%d" % p, "%04d.png" % f))
    if frames is not None:
        os.makedirs(os.path.join(out_dir, "image"), exist_ok=True)
        for f, path in enumerate(frames):
            img = Image.open(path).convert("RGB")
            if scale_factor > 1:               # whole boxes only: (H // s, W // s), like the masks
                img = img.reduce(scale_factor, box=(0, 0, img.size[0] // scale_factor * scale_factor,
                                                    img.size[1] // scale_factor * scale_factor))
            if (img.size[1], img.size[0]) != tuple(scene["img_size"]):
                raise ValueError(f"{path}: {img.size[1]} x {img.size[0]} after the reduction, the masks are {scene['img_size']}")
            img.save(os.path.join(out_dir, "image", "%04d.png" % f))


def write_overlays(out_dir, verts, faces, cam16, img_size, frames_per_call=None):
    """The QC images of a written scene folder (the reference's init_smpl_image/ and init_refined_smpl/ folders,
    preprocessing_multiple_trace.py:330-342, 496-510), over the folder's own image/%04d.png: overlay/<p>/%04d.png = person p in
    'normal' colours, overlay/all/%04d.png = all persons tinted with mesh_losses.COLOR_DICT and z-tested against each other
    (overlay.render_overlays).  verts (F, P, V, 3): the posed bodies v'; cam16: the camera of the silhouettes -- the scene's written
    intrinsics and [Rt | 0]: the written cam_f = K4 [Rt | -Rt shift_f] acts on v' + shift_f, the shift cancels, and with the
    silhouettes' own arithmetic an overlay covers exactly the pixels of the undilated mask.  frames_per_call bounds the frames held
    at once (default 16)."""
    from PIL import Image
    from . import overlay as OV
    from .mesh_losses import COLOR_DICT
    F, P = verts.shape[:2]
    H, W = img_size
    dev = verts.device
    step = 16 if frames_per_call is None else max(1, int(frames_per_call))
    adj = tuple(torch.from_numpy(a).to(dev) for a in OV.vertex_adjacency(faces, verts.shape[2]))
    tint = torch.tensor([COLOR_DICT[p % len(COLOR_DICT)] for p in range(P)], dtype=torch.float32, device=dev) / 255.0
    for name in ["all"] + ["%d" % p for p in range(P)]:
        os.makedirs(os.path.join(out_dir, "overlay", name), exist_ok=True)
    for f0 in range(0, F, step):
        f1 = min(F, f0 + step)
        n = f1 - f0
        img = np.stack([np.asarray(Image.open(os.path.join(out_dir, "image", "%04d.png" % f)).convert("RGB")) for f in range(f0, f1)])
        if img.shape[1:3] != (H, W):
            raise ValueError(f"image/: {img.shape[1]} x {img.shape[2]}, the scene is {H} x {W}")
        fr = torch.from_numpy(img).to(dev)
        v = verts[f0:f1].reshape(n * P, -1, 3).contiguous()
        nrm = OV.vertex_normals(v, faces, adj)
        image_of = [i // P for i in range(n * P)]
        pics = {"all": OV.render_overlays((v, faces, OV.vertex_colors(nrm, "tint", tint=tint.repeat(n, 1))), image_of, cam16, H, W,
                                          frames=fr)}
        col = OV.vertex_colors(nrm, "normal").reshape(n, P, -1, 3)
        for p in range(P):
            pics["%d" % p] = OV.render_overlays((verts[f0:f1, p].contiguous(), faces, col[:, p].contiguous()), list(range(n)), cam16,
                                                H, W, frames=fr)
        for name, pic in pics.items():
            pic = pic.cpu().numpy()
            for i in range(n):
                Image.fromarray(pic[i]).save(os.path.join(out_dir, "overlay", name, "%04d.png" % (f0 + i)))


# ------------------------------------------------------------------------------------------------ between detector output and refine
def estimate_translation(joints3d, joints2d, intrinsics, weights=None):
    """The initial translation of `mask` mode (:316-319).  The reference calls cv2.solvePnPRansac on the body's joints and keeps only
    tvec: random, third party, and its rotation is thrown away.  Here: the deterministic translation-only weighted least squares --
    per joint  fx (X + tx) - (u - cx) (Z + tz) = 0  and  fy (Y + ty) - (v - cy) (Z + tz) = 0 , solved through the 3 x 3 normal
    equations in float64 (torch.linalg.solve).  On exact projections both give the true translation; with outliers RANSAC would
    reject what this weights.  joints3d (N, J, 3), joints2d (N, J, 2), weights (N, J) or None -> (N, 3) float64."""
    X = torch.as_tensor(_np(joints3d), dtype=torch.float64)
    uv = torch.as_tensor(_np(joints2d), dtype=torch.float64)
    if X.dim() != 3 or X.shape[-1] != 3 or uv.shape != X.shape[:2] + (2,):
        raise ValueError(f"expected joints3d (N, J, 3) and joints2d (N, J, 2), got {tuple(X.shape)}, {tuple(uv.shape)}")
    K = np.asarray(intrinsics, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    w = torch.ones(X.shape[:2], dtype=torch.float64) if weights is None else torch.as_tensor(_np(weights), dtype=torch.float64)
    a, b = uv[..., 0] - cx, uv[..., 1] - cy
    z, o = torch.zeros_like(a), torch.ones_like(a)
    A = torch.stack([torch.stack([fx * o, z, -a], -1), torch.stack([z, fy * o, -b], -1)], 2)          # (N, J, 2, 3)
    rhs = torch.stack([a * X[..., 2] - fx * X[..., 0], b * X[..., 2] - fy * X[..., 1]], -1)          # (N, J, 2)
    AtA = torch.einsum("nj,njri,njrk->nik", w, A, A)
    Atb = torch.einsum("nj,njri,njr->ni", w, A, rhs)
    return torch.linalg.solve(AtA, Atb).numpy()


def interpolate_missing(pose, trans, frame_ids):
    """`interpolate` (:48-69): the frames named in frame_ids are replaced by an interpolation of the others -- per joint a
    scipy RotationSpline over the available frames, a CubicSpline for the translation.  pose (F, 72), trans (F, 3) -> new arrays
    (float64); every other frame keeps its bits."""
    from scipy.interpolate import CubicSpline
    from scipy.spatial.transform import Rotation, RotationSpline
    pose, trans = np.array(_np(pose), np.float64), np.array(_np(trans), np.float64)
    F = pose.shape[0]
    ids = np.unique(np.asarray(list(frame_ids), dtype=np.int64))
    if ids.size == 0:
        return pose, trans
    if ids.min() < 0 or ids.max() >= F:
        raise ValueError(f"frame_ids outside 0 .. {F - 1}")
    avail = np.ones(F, dtype=bool)
    avail[ids] = False
    t_in = np.arange(F)[avail]
    if t_in.size < 2:
        raise ValueError("interpolation needs at least two available frames")
    ps = pose.reshape(F, -1, 3)
    for j in range(ps.shape[1]):
        ps[ids, j] = RotationSpline(t_in, Rotation.from_rotvec(ps[avail, j]))(ids).as_rotvec()
    trans[ids] = CubicSpline(t_in, trans[avail], axis=0)(ids)
    return ps.reshape(F, -1), trans


def match_detections(detections, mask_centres, max_cost=200.0):
    """run_openpose_multiple_trace.py:83-96: which detection belongs to which tracked person.  detections: per frame an (n_f, K, 3)
    array of (u, v, confidence); mask_centres (F, P, 2) = (col, row) centres of the persons' raw masks (mask_stats 'centre').  A
    detection's centre is its confidence-weighted mean keypoint, the cost of a pair the distance of the two centres, the assignment
    scipy's linear_sum_assignment; a person whose assignment costs max_cost or more (or who gets none) has a zero row.
    -> (F, P, K, 3) float32."""
    from scipy.optimize import linear_sum_assignment
    cen = np.asarray(_np(mask_centres), np.float64)
    F, P = cen.shape[:2]
    if len(detections) != F:
        raise ValueError(f"detections: expected {F} frames, got {len(detections)}")
    K = next((np.asarray(d).shape[1] for d in detections if np.asarray(d).ndim == 3 and np.asarray(d).shape[0]), 0)
    out = np.zeros((F, P, K, 3), dtype=np.float32)
    for f in range(F):
        det = np.asarray(detections[f], np.float64).reshape(-1, K, 3) if K else np.zeros((0, 0, 3))
        if det.shape[0] == 0:
            continue
        w = det[..., 2]
        ws = w.sum(1)
        dc = np.where(ws[:, None] > 0, (det[..., :2] * w[..., None]).sum(1) / np.where(ws > 0, ws, 1.0)[:, None], np.inf)
        cost = np.linalg.norm(dc[:, None, :] - cen[f][None, :, :], axis=-1)                 # (n, P)
        cost = np.where(np.isfinite(cost), cost, 1e18)                                         # no confidence / no mask: never chosen
        rows, cols = linear_sum_assignment(cost)
        for r, c in zip(rows, cols):
            if cost[r, c] < max_cost:
                out[f, c] = det[r]
    return out


def gate_second_set(first, second, zero=range(19), pairs=((15, 14, (19, 20, 21)), (16, 11, (22, 23, 24))), max_px=30.0):
    """:412-419: the second keypoint set (OpenPose's 25 beside ViTPose's 17) keeps only what the first lacks -- the confidences listed
    in `zero` are cleared, and for each (i, j, foot) the `foot` confidences are cleared where |first[i] - second[j]| > max_px (the
    two detectors disagree about the ankle the feet hang on).  first (F, P, K1, 3), second (F, P, 25, 3) -> a new array like second,
    to be passed as second_set['keypoints'] of refine_sequence."""
    first = np.asarray(_np(first), np.float64)
    out = np.array(_np(second), copy=True)
    out[..., list(zero), 2] = 0
    for i, j, foot in pairs:
        far = np.linalg.norm(first[..., i, :2] - np.asarray(out[..., j, :2], np.float64), axis=-1) > max_px
        for k in foot:
            out[..., k, 2] = np.where(far, 0, out[..., k, 2])
    return out
