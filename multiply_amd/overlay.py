"""Shaded mesh overlays for a batch of meshes on the device: the QC images of preprocessing and testing (csrc/overlay.hip).

The reference writes such a picture at every preprocessing stage (preprocessing_multiple_trace.py:330-342, 496-510) and for the
reconstructed meshes (ait_viewer_vis/vis_mesh_image.py), one mesh per pytorch3d call.  Here a whole sequence is one call per
`images_per_call` chunk: vertex normals (mp_mesh_vertex_normals), vertex colours (mp_overlay_vertex_colors) and the z-tested,
blended, keypoint-decorated images (mp_overlay_batch).  The rule is stated in include/multiply_hip.h and DESIGN section 6n.

`vertex_adjacency`, `record_table` and the argument checks run on the host and import without a device.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import hip
from .render import Z_CLIP

MODES = {"normal": 0, "shade": 1, "tint": 2}          # = MP_OVERLAY_* of include/multiply_hip.h
BLOCK = 256                                           # faces per block of mp_overlay_batch's grid
MAX_FACES = 2 ** 32 - 2                               # the key's low word; 2^32 - 1 marks an empty pixel
MAX_PIXELS = 2 ** 31 - 2
MAX_KP_RADIUS = 4096


class MpOverlayMesh(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("faces", C.c_void_p), ("colors", C.c_void_p), ("n_verts", C.c_int), ("n_faces", C.c_int),
                ("image", C.c_int), ("block0", C.c_int), ("face_base", C.c_uint), ("pad_", C.c_int)]


# ------------------------------------------------------------------------------------------------ host side
def vertex_adjacency(faces, n_verts):
    """faces (F, 3) integers, n_verts -> (adj_ptr (n_verts + 1,), adj_face (3 F,)) int32 numpy arrays: the faces that contain
    vertex v are adj_face[adj_ptr[v] : adj_ptr[v + 1]], ascending, once per corner (a repeated face counts twice, as in
    render_mesh_recon's index_add).  Built once per topology."""
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces).reshape(-1, 3).astype(np.int64)
    n_verts = int(n_verts)
    if n_verts < 0:
        raise ValueError(f"n_verts must not be negative, got {n_verts}")
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise ValueError(f"faces index vertices {int(f.min())} .. {int(f.max())}, the mesh has {n_verts}")
    if 3 * f.shape[0] > 2 ** 31 - 1:
        raise ValueError("too many faces for an int32 adjacency")
    corner = f.reshape(-1)
    order = np.argsort(corner, kind="stable")              # stable: corners of a vertex stay in ascending face order
    adj_face = (order // 3).astype(np.int32)
    adj_ptr = np.zeros(n_verts + 1, dtype=np.int64)
    np.cumsum(np.bincount(corner, minlength=n_verts), out=adj_ptr[1:])
    return adj_ptr.astype(np.int32), adj_face


def record_table(entries, n_images):
    """entries: one (verts_ptr, faces_ptr, colors_ptr, n_verts, n_faces, image) per mesh, in drawing order -> (ctypes array of
    MpOverlayMesh, total_blocks, total_faces).  face_base / block0 are the exclusive prefix sums of n_faces / ceil(n_faces /
    256).  ValueError: an image outside [0, n_images), negative sizes, 2^32 - 1 faces or more in all."""
    table = (MpOverlayMesh * max(len(entries), 1))()
    blocks = faces = 0
    for i, (vp, fp, cp, nv, nf, image) in enumerate(entries):
        nv, nf, image = int(nv), int(nf), int(image)
        if nv < 0 or nf < 0:
            raise ValueError(f"mesh {i}: negative size ({nv} vertices, {nf} faces)")
        if not 0 <= image < n_images:
            raise ValueError(f"mesh {i}: image {image} outside [0, {n_images})")
        if faces + nf > MAX_FACES:
            raise ValueError(f"{faces + nf} faces in one call: a face id is 32 bits (at most {MAX_FACES}); lower images_per_call")
        table[i] = MpOverlayMesh(vp, fp, cp, nv, nf, image, blocks, faces, 0)
        blocks += (nf + BLOCK - 1) // BLOCK
        faces += nf
    if blocks > 2 ** 31 - 1:
        raise ValueError("too many face blocks in one call; lower images_per_call")
    return table, blocks, faces


def _check_paint(H, W, opacity, kp_radius):
    if int(H) < 1 or int(W) < 1:
        raise ValueError(f"image size must be positive, got {H} x {W}")
    if not 0.0 <= float(opacity) <= 1.0:
        raise ValueError(f"opacity must lie in [0, 1], got {opacity}")
    if not 0 <= int(kp_radius) <= MAX_KP_RADIUS:
        raise ValueError(f"kp_radius must lie in [0, {MAX_KP_RADIUS}], got {kp_radius}")


def _cams(cams, M):
    c = np.asarray(cams.detach().cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float32)
    if c.size % 16 or c.size == 0:
        raise ValueError(f"cams: expected (16,), (1, 16) or (M, 16) floats, got shape {c.shape}")
    c = np.ascontiguousarray(c.reshape(-1, 16))
    if c.shape[0] not in (1, M):
        raise ValueError(f"cams: {c.shape[0]} cameras for {M} images (one for all, or one each)")
    return c


# ------------------------------------------------------------------------------------------------ device wrappers
def vertex_normals(verts, faces, adjacency=None):
    """verts (N, V, 3) or (V, 3) device fp32, faces (F, 3) -> normals of the same shape: the normalised (eps 1e-6) sum of
    cross(v1 - v0, v2 - v0) over the faces of each vertex, summed in ascending face order (mp_mesh_vertex_normals).
    adjacency: vertex_adjacency(faces, V) when the caller keeps it (host arrays or device tensors)."""
    hip.require_device()
    if verts.dim() not in (2, 3) or verts.shape[-1] != 3:
        raise ValueError(f"verts: expected (N, V, 3) or (V, 3), got {tuple(verts.shape)}")
    v = verts.detach().float().contiguous()
    V = v.shape[-2]
    N = 1 if v.dim() == 2 else v.shape[0]
    if N * V > MAX_PIXELS:
        raise ValueError("too many vertices in one call")
    if adjacency is None:
        adjacency = vertex_adjacency(faces, V)
    ptr, adj = (torch.as_tensor(a).to(device=v.device, dtype=torch.int32).contiguous() for a in adjacency)
    if ptr.numel() != V + 1:
        raise ValueError(f"adjacency is for {ptr.numel() - 1} vertices, the meshes have {V}")
    f = torch.as_tensor(faces).reshape(-1, 3).to(device=v.device, dtype=torch.int32).contiguous()
    if adj.numel() != 3 * f.shape[0]:
        raise ValueError(f"adjacency lists {adj.numel()} corners, the faces have {3 * f.shape[0]}")
    out = torch.empty_like(v)
    hip.lib().mp_mesh_vertex_normals(v, N, V, f, f.shape[0], ptr, adj, out, hip.stream())
    return out


def vertex_colors(normals, mode, tint=None, light=(0, 0, 1), ambient=0.3):
    """normals (N, V, 3) or (V, 3) -> colours of the same shape (mp_overlay_vertex_colors).  mode 'normal': (0.5 n + 0.5) with
    the channels reversed, as the reference; 'shade': max(n . light, 0) on all channels; 'tint': tint[n] (ambient + (1 - ambient)
    max(n . light, 0)) with tint (N, 3) (or (3,) for all meshes)."""
    hip.require_device()
    if mode not in MODES:
        raise ValueError(f"mode must be one of {tuple(MODES)}, got {mode!r}")
    if normals.dim() not in (2, 3) or normals.shape[-1] != 3:
        raise ValueError(f"normals: expected (N, V, 3) or (V, 3), got {tuple(normals.shape)}")
    n = normals.detach().float().contiguous()
    V = n.shape[-2]
    N = 1 if n.dim() == 2 else n.shape[0]
    t = None
    if mode == "tint":
        if tint is None:
            raise ValueError("mode 'tint' needs a tint")
        t = torch.as_tensor(tint, dtype=torch.float32).to(n.device).reshape(-1, 3)
        if t.shape[0] == 1:
            t = t.expand(N, 3)
        if t.shape[0] != N:
            raise ValueError(f"tint: {t.shape[0]} colours for {N} meshes")
        t = t.contiguous()
    lx, ly, lz = (float(x) for x in light)
    out = torch.empty_like(n)
    hip.lib().mp_overlay_vertex_colors(n, N, V, MODES[mode], t, lx, ly, lz, float(ambient), out, hip.stream())
    return out


def _mesh_list(meshes, device):
    """-> [(verts (V, 3), faces (F, 3) int32, colors (V, 3))] contiguous on the device; shared tensors stay shared"""
    if isinstance(meshes, tuple) and len(meshes) == 3 and isinstance(meshes[0], torch.Tensor) and meshes[0].dim() == 3:
        verts, faces, colors = meshes
        v = verts.detach().float().contiguous().to(device)
        c = colors.detach().float().contiguous().to(device)
        if v.shape[-1] != 3 or c.shape != v.shape:
            raise ValueError(f"verts {tuple(v.shape)} and colors {tuple(c.shape)}: expected the same (N, V, 3)")
        f = torch.as_tensor(faces).reshape(-1, 3).to(device=device, dtype=torch.int32).contiguous()
        return [(v[i], f, c[i]) for i in range(v.shape[0])]
    out, shared = [], {}
    for i, (verts, faces, colors) in enumerate(meshes):
        v = verts.detach().reshape(-1, 3).float().contiguous().to(device)
        c = colors.detach().reshape(-1, 3).float().contiguous().to(device)
        if c.shape != v.shape:
            raise ValueError(f"mesh {i}: one colour per vertex ({tuple(v.shape)} vertices, {tuple(c.shape)} colours)")
        key = id(faces)
        if key not in shared:
            shared[key] = torch.as_tensor(faces).reshape(-1, 3).to(device=device, dtype=torch.int32).contiguous()
        out.append((v, shared[key], c))
    return out


def render_overlays(meshes, image_of, cams, H, W, frames=None, background=(255, 255, 255), opacity=1.0, keypoints=None,
                    kp_rgb=None, kp_conf=0.0, kp_radius=5, images_per_call=None, want_owner=False, n_images=None, device=None):
    """Draws meshes into M images of H x W (mp_overlay_batch) -> out (M, H, W, 3) uint8 [, owner (M, H, W) int32 with want_owner].

    meshes       (verts (N, V, 3), faces (F, 3), colors (N, V, 3)) -- one topology, e.g. SMPL bodies over a sequence -- or a list
                 of (verts (V_i, 3), faces (F_i, 3), colors (V_i, 3)) triples; world space; colours in [0, 1]
    image_of     the image each mesh is drawn into; meshes of one image are z-tested against each other (ties: the earlier)
    cams         (16,) / (1, 16) for all images or (M, 16): R (9, row major), T (3), fx, fy, cx, cy -- mp_raster_zbuf's layout
    frames       (M, H, W, 3) uint8 to draw over, or None: the `background` colour
    opacity      out = floor(fmaf(opacity, mesh byte - frame byte, frame byte) + 0.5) on covered pixels
    keypoints    (M, K, 3) = x, y, confidence with kp_rgb (K, 3) bytes: integer discs of kp_radius around (floor x, floor y) for
                 confidence > kp_conf and finite x, y, painted last, the highest index on top
    images_per_call  bounds the scratch (8 bytes per pixel, 4 per face of a call); an image's bytes do not depend on it
    n_images     M when neither frames, keypoints nor cams say it (default then: max(image_of) + 1)
    Limit violations raise ValueError before any launch."""
    _check_paint(H, W, opacity, kp_radius)
    H, W = int(H), int(W)
    if images_per_call is not None and int(images_per_call) < 1:
        raise ValueError(f"images_per_call must be at least 1, got {images_per_call}")
    image_of = [int(i) for i in (image_of.tolist() if hasattr(image_of, "tolist") else image_of)]
    if frames is not None:
        if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != (H, W, 3):
            raise ValueError(f"frames: expected (M, {H}, {W}, 3) uint8, got {tuple(frames.shape)} {frames.dtype}")
    if keypoints is not None and (keypoints.dim() != 3 or keypoints.shape[-1] != 3):
        raise ValueError(f"keypoints: expected (M, K, 3), got {tuple(keypoints.shape)}")
    ncam_rows = np.asarray(cams.detach().cpu() if isinstance(cams, torch.Tensor) else cams).size // 16
    if n_images is not None:
        M = int(n_images)
    elif frames is not None:
        M = frames.shape[0]
    elif keypoints is not None:
        M = keypoints.shape[0]
    elif ncam_rows > 1:
        M = ncam_rows
    else:
        M = max(image_of) + 1 if image_of else 0
    for name, t in (("frames", frames), ("keypoints", keypoints)):
        if t is not None and t.shape[0] != M:
            raise ValueError(f"{name}: {t.shape[0]} images, expected {M}")
    if M > 0:
        cam = _cams(cams, M)
    K = 0 if keypoints is None else keypoints.shape[1]
    if K > 0:
        if kp_rgb is None:
            raise ValueError("keypoints need kp_rgb (K, 3)")
        rgb = torch.as_tensor(kp_rgb).reshape(-1, 3)
        if rgb.shape[0] != K or int(rgb.min()) < 0 or int(rgb.max()) > 255:
            raise ValueError(f"kp_rgb: expected ({K}, 3) bytes")
    bg = [int(x) for x in background]
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError(f"background: expected 3 bytes, got {background}")
    hip.require_device()
    if device is None:
        first = meshes[0] if isinstance(meshes, tuple) else (meshes[0][0] if len(meshes) else None)
        device = first.device if isinstance(first, torch.Tensor) and first.is_cuda else (
            frames.device if frames is not None and frames.is_cuda else torch.device("cuda"))
    device = torch.device(device)
    ml = _mesh_list(meshes, device)
    if len(ml) != len(image_of):
        raise ValueError(f"{len(ml)} meshes, {len(image_of)} entries of image_of")
    step = max(M, 1) if images_per_call is None else int(images_per_call)
    step = max(1, min(step, MAX_PIXELS // (H * W)))
    # everything that can be refused is refused here, before the first launch
    checked, chunks = {}, []
    for s in range(0, M, step):
        e = min(M, s + step)
        idx = [i for i, im in enumerate(image_of) if s <= im < e]
        entries = [(ml[i][0].data_ptr(), ml[i][1].data_ptr(), ml[i][2].data_ptr(), ml[i][0].shape[0], ml[i][1].shape[0],
                    image_of[i] - s) for i in idx]
        chunks.append((s, e) + record_table(entries, e - s) + (len(idx),))
    for i, im in enumerate(image_of):
        if not 0 <= im < M:
            raise ValueError(f"mesh {i}: image {im} outside [0, {M})")
        v, f, _ = ml[i]
        key = (f.data_ptr(), f.shape[0], v.shape[0])
        if key not in checked and f.numel():
            lo, hi = int(f.min()), int(f.max())
            if lo < 0 or hi >= v.shape[0]:
                raise ValueError(f"mesh {i}: faces index vertices {lo} .. {hi}, the mesh has {v.shape[0]}")
            checked[key] = True
    out = torch.empty(M, H, W, 3, dtype=torch.uint8, device=device)
    owner = torch.empty(M, H, W, dtype=torch.int32, device=device) if want_owner else None
    if M == 0:
        return (out, owner) if want_owner else out
    fr = None if frames is None else frames.to(device).contiguous()
    kp = None if K == 0 else keypoints.detach().float().to(device).contiguous()
    rgb = None if K == 0 else rgb.to(device=device, dtype=torch.uint8).contiguous()
    bg_host = (C.c_ubyte * 3)(*bg)
    keys = torch.empty(min(step, M) * H * W, dtype=torch.int64, device=device)
    big = torch.empty(1 + max(c[4] for c in chunks), dtype=torch.int32, device=device)
    cam_dev = torch.empty(cam.shape[0] * 16, dtype=torch.float32, device=device)
    L = hip.lib()
    for s, e, table, blocks, faces, n_rec in chunks:
        tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(device) if n_rec else None
        c = cam if cam.shape[0] == 1 else np.ascontiguousarray(cam[s:e])
        L.mp_overlay_batch(tab, n_rec, blocks, faces, e - s, H, W, c.ctypes.data_as(C.c_void_p), c.shape[0], Z_CLIP,
                           None if fr is None else fr[s:e], C.cast(bg_host, C.c_void_p), float(opacity),
                           None if kp is None else kp[s:e], K, rgb, float(kp_conf), int(kp_radius), keys, big, cam_dev, out[s:e],
                           None if owner is None else owner[s:e], hip.stream())
    if owner is not None and step < M:
        # record indices of a chunk's table -> indices into `meshes`
        for s, e, _, _, _, n_rec in chunks:
            idx = torch.tensor([i for i, im in enumerate(image_of) if s <= im < e] + [-1], dtype=torch.int32, device=device)
            o = owner[s:e]
            o.copy_(idx[o.long()])                        # -1 indexes the trailing -1
    return (out, owner) if want_owner else out


def write_fit_overlays(dst, servers, fit, keypoints, kmap, camera, frames, conf_threshold=0.6, kp_radius=3, frames_per_call=16):
    """The QC images of a keypoint fit (the reference's init_smpl_image/ and init_refined_smpl/,
    preprocessing_multiple_trace.py:330-342, 496-510): dst/<p>/%04d.png = the body of person p with `fit`'s parameters in 'normal'
    colours over the frame, the detected keypoints whose confidence exceeds conf_threshold in red and, above them, the model's
    projected keypoints (keypoint_fit.project_keypoints) in green.  servers: one SMPLServer per person or one for all; fit: dict of
    pose (F, P, 72), trans (F, P, 3), shape (F, P, 10) in `camera`'s space; keypoints (F, P, K, 3) in kmap's order; camera:
    what keypoint_fit takes (intrinsics and an optional extrinsic); frames: F image paths."""
    from PIL import Image
    from . import keypoint_fit as KF
    pose, trans, shape = (torch.as_tensor(np.asarray(_host(fit[k]), np.float32)) for k in ("pose", "trans", "shape"))
    F, P = pose.shape[:2]
    if len(frames) != F:
        raise ValueError(f"frames: expected {F} paths, got {len(frames)}")
    servers = list(servers) if isinstance(servers, (list, tuple)) else [servers]
    if len(servers) not in (1, P):
        raise ValueError(f"servers: expected one per person ({P}) or one for all, got {len(servers)}")
    kp = torch.as_tensor(np.asarray(_host(keypoints), np.float32))
    K = kmap.K
    if tuple(kp.shape) != (F, P, K, 3):
        raise ValueError(f"keypoints: expected ({F}, {P}, {K}, 3), got {tuple(kp.shape)}")
    row = KF.camera_rows(camera, 1)[0].double().numpy()                     # fx, fy, cx, cy, E (3, 4)
    E = row[4:].reshape(3, 4)
    cam16 = list(E[:, :3].reshape(-1)) + list(E[:, 3]) + list(row[:4])
    proj, _ = KF.project_keypoints(servers, KF.pack_params(pose, trans, shape).reshape(F * P, -1), kmap, camera,
                                   row_server=None if len(servers) == 1 else np.tile(np.arange(P), F))
    proj = proj.reshape(F, P, K, 2).float().cpu()
    shown = torch.cat([proj, torch.full((F, P, K, 1), float(conf_threshold) + 1.0)], -1)      # always above the threshold
    marks = torch.cat([kp, shown], 2)                                                           # (F, P, 2 K, 3): green over red
    rgb = np.array([[255, 0, 0]] * K + [[0, 255, 0]] * K, dtype=np.uint8)
    servers = servers * P if len(servers) == 1 else servers
    dev = servers[0].param_canonical.device
    with Image.open(frames[0]) as im:
        W, H = im.size
    step = max(1, int(frames_per_call))
    for p in range(P):
        os.makedirs(os.path.join(dst, "%d" % p), exist_ok=True)
        faces = torch.from_numpy(np.ascontiguousarray(servers[p].faces)).to(dev)
        prm = torch.cat([torch.ones(F, 1), trans[:, p], pose[:, p], shape[:, p]], 1)
        verts = servers[p].pose_batch(prm, absolute=True, want=("verts",))["verts"]
        adj = tuple(torch.from_numpy(a).to(dev) for a in vertex_adjacency(faces, verts.shape[1]))
        for f0 in range(0, F, step):
            f1 = min(F, f0 + step)
            img = torch.from_numpy(np.stack([np.asarray(Image.open(frames[f]).convert("RGB")) for f in range(f0, f1)])).to(dev)
            v = verts[f0:f1].contiguous()
            col = vertex_colors(vertex_normals(v, faces, adj), "normal")
            pics = render_overlays((v, faces, col), list(range(f1 - f0)), cam16, H, W, frames=img, keypoints=marks[f0:f1, p].to(dev),
                                   kp_rgb=rgb, kp_conf=float(conf_threshold), kp_radius=kp_radius).cpu().numpy()
            for i in range(f1 - f0):
                Image.fromarray(pics[i]).save(os.path.join(dst, "%d" % p, "%04d.png" % (f0 + i)))


def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
