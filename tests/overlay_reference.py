"""float64 numpy restatement of the overlay rule (include/multiply_hip.h): vertex normals, the three colour
modes, colour / byte / blend from a given (face, barycentrics), the keypoint discs, and -- for the CPU tests and for choosing
the fixture -- the rasterisation rule itself.  The project's own; reads nothing outside the repository.  Also the base scene
of tests/test_overlay_gpu.py, so that the CPU test can check the conditions the GPU test relies on."""
import numpy as np

U = 2.0 ** -24                       # fp32 unit roundoff
Z_CLIP = 1e-6
K_EPS = 1e-8
MARGIN = 2.0 ** -12                  # see test_overlay_gpu.test_colours: distance of 255 c from an integer below which a byte may flip


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(centre=(0.0, 0.0, 0.0), radius=1.0, subdivisions=1):
    """subdivisions = 1: 42 vertices, 80 faces, outward winding"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius + np.asarray(centre, dtype=np.float64)).astype(np.float32), np.array(f, dtype=np.int32)


# ------------------------------------------------------------------------------------------------ normals and colours
def vertex_normals(verts, faces):
    """verts (V, 3), faces (F, 3) -> normals (V, 3) float64 = s / max(|s|, 1e-6), s = sum over the corners at v of cross(v1 - v0,
    v2 - v0); and `mag` (V, 3): the sum of the absolute values of the two products of every component of every term, and `cnt`
    (V,): the number of terms -- what an fp32 error bound is made of."""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces).reshape(-1, 3)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    fn = np.cross(a, b)
    fm = np.abs(a[:, [1, 2, 0]] * b[:, [2, 0, 1]]) + np.abs(a[:, [2, 0, 1]] * b[:, [1, 2, 0]])
    s, mag, cnt = np.zeros_like(v), np.zeros_like(v), np.zeros(v.shape[0])
    for k in range(3):
        np.add.at(s, f[:, k], fn)
        np.add.at(mag, f[:, k], fm)
        np.add.at(cnt, f[:, k], 1)
    ln = np.maximum(np.linalg.norm(s, axis=1, keepdims=True), 1e-6)
    return s / ln, mag, cnt


def normals_bound(verts, faces):
    """per-element bound on |fp32 normals - float64 normals| from the operand magnitudes.  Each component of a term is a
    difference of two products of differences: four roundings of relative size U on its two products (two subtractions, the
    product, the combination; fewer when contracted) => 4 U mag; adding cnt terms in sequence: (cnt - 1) U mag more.  So
    E = (cnt + 3) U mag bounds the error of s.  n = s / len with len = |s|: |d len| <= |E| + 3 U len (the three squares and
    the root), and the division adds U: |d n_i| <= E_i / len + |n_i| |E| / len + 5 U |n_i|.  Doubled for the second-order
    terms."""
    v, f = np.asarray(verts, dtype=np.float64), np.asarray(faces).reshape(-1, 3)
    n, mag, cnt = vertex_normals(v, f)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    s = np.zeros_like(v)
    for k in range(3):
        np.add.at(s, f[:, k], np.cross(a, b))
    ln = np.maximum(np.linalg.norm(s, axis=1, keepdims=True), 1e-6)
    E = (cnt[:, None] + 3) * U * mag
    return 2.0 * (E / ln + np.abs(n) * np.linalg.norm(E, axis=1, keepdims=True) / ln + 5 * U * np.abs(n))


def vertex_colors(normals, mode, tint=None, light=(0.0, 0.0, 1.0), ambient=0.3):
    """normals (N, V, 3) -> (colours (N, V, 3) float64, bound (N, V, 3) on the fp32 kernel's error from the operand
    magnitudes).  light / ambient / tint are taken at their fp32 values, as the kernel receives them."""
    n = np.asarray(normals, dtype=np.float64)
    l = np.asarray(light, dtype=np.float32).astype(np.float64)
    a = float(np.float32(ambient))
    if mode == "normal":
        c = (n * 0.5 + 0.5)[..., ::-1]
        return c, 2 * U * (np.abs(n[..., ::-1]) * 0.5 + 0.5)            # one product (exact), one sum
    dot = n @ l
    d = np.maximum(dot, 0.0)
    dd = 4 * U * (np.abs(n) @ np.abs(l))                                  # three products, two sums
    if mode == "shade":
        return np.repeat(d[..., None], 3, -1), np.repeat(dd[..., None], 3, -1)
    t = np.asarray(tint, dtype=np.float32).astype(np.float64).reshape(-1, 1, 3)
    s = a + (1.0 - a) * d
    ds = abs(1.0 - a) * dd + 4 * U * (abs(a) + abs(1.0 - a) * d)          # 1 - a, the product, the sum
    return t * s[..., None], 2.0 * np.abs(t) * (ds + U * np.abs(s))[..., None]


# ------------------------------------------------------------------------------------------------ pixels
def mesh_value(bary, face_colors):
    """v = 255 clamp(b0 c0 + b1 c1 + b2 c2, 0, 1): bary (..., 3), face_colors (..., 3 corners, 3 channels) -> (..., 3)"""
    c = np.einsum("...k,...kc->...c", np.asarray(bary, dtype=np.float64), np.asarray(face_colors, dtype=np.float64))
    return 255.0 * np.clip(c, 0.0, 1.0)


def blend(v, frame, opacity):
    """mesh byte m = floor(v), out = floor(opacity (m - f) + f + 0.5) with opacity at its fp32 value"""
    m = np.floor(v)
    f = np.asarray(frame, dtype=np.float64)
    return np.floor(float(np.float32(opacity)) * (m - f) + f + 0.5).astype(np.uint8)


def paint_keypoints(image, keypoints, kp_rgb, kp_conf, radius):
    """image (H, W, 3) uint8, keypoints (K, 3) = x, y, conf, kp_rgb (K, 3): the integer discs, ascending so the highest wins"""
    out = image.copy()
    H, W = out.shape[:2]
    kp_conf = float(np.float32(kp_conf))                      # the threshold at its fp32 value, as the kernel receives it
    r, c = np.mgrid[0:H, 0:W]
    for k, (x, y, conf) in enumerate(np.asarray(keypoints, dtype=np.float64)):
        if not (conf > kp_conf) or not np.isfinite(x) or not np.isfinite(y):
            continue
        inside = (c - int(np.floor(x))) ** 2 + (r - int(np.floor(y))) ** 2 <= int(radius) ** 2
        out[inside] = np.asarray(kp_rgb)[k]
    return out


def rasterize(meshes, cam16, H, W):
    """the visibility rule in float64: meshes = [(verts, faces)] of ONE image in record order -> (owner (H, W) record or -1,
    face (H, W) local face, bary (H, W, 3)).  Nearest depth, ties to the earlier record then the lower face."""
    cam = np.asarray(cam16, dtype=np.float64)
    R, T, fx, fy, cx, cy = cam[:9].reshape(3, 3), cam[9:12], cam[12], cam[13], cam[14], cam[15]
    py, px = np.mgrid[0:H, 0:W] + 0.5
    depth = np.full((H, W), np.inf)
    owner, face, bary = -np.ones((H, W), int), -np.ones((H, W), int), -np.ones((H, W, 3))
    edge = lambda ax, ay, bx, by: (px - ax) * (by - ay) - (py - ay) * (bx - ax)
    for ri, (verts, faces) in enumerate(meshes):
        X = np.asarray(verts, dtype=np.float64) @ R.T + T
        with np.errstate(all="ignore"):
            x, y, z = fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy, X[:, 2]
        for fi, (i0, i1, i2) in enumerate(np.asarray(faces).reshape(-1, 3)):
            if not min(z[i0], z[i1], z[i2]) >= Z_CLIP:
                continue
            area = (x[i2] - x[i0]) * (y[i1] - y[i0]) - (y[i2] - y[i0]) * (x[i1] - x[i0])
            if not abs(area) > K_EPS:
                continue
            a = area + K_EPS
            w0, w1, w2 = edge(x[i1], y[i1], x[i2], y[i2]) / a, edge(x[i2], y[i2], x[i0], y[i0]) / a, edge(x[i0], y[i0], x[i1], y[i1]) / a
            t0, t1, t2 = w0 * z[i1] * z[i2], z[i0] * w1 * z[i2], z[i0] * z[i1] * w2
            d = np.maximum(t0 + t1 + t2, K_EPS)
            b = np.stack([t0 / d, t1 / d, t2 / d], -1)
            pz = b @ np.array([z[i0], z[i1], z[i2]])
            win = (w0 > 0) & (w1 > 0) & (w2 > 0) & (pz >= 0) & (pz < depth)          # strict: an equal depth keeps the earlier
            depth[win], owner[win], face[win], bary[win] = pz[win], ri, fi, b[win]
    return owner, face, bary


def render(meshes, cam16, H, W, frame, opacity=1.0, keypoints=None, kp_rgb=None, kp_conf=0.0, radius=5):
    """one image by the whole rule: meshes = [(verts, faces, colors)] -> (out (H, W, 3) uint8, owner (H, W), v (H, W, 3))"""
    owner, face, bary = rasterize([(m[0], m[1]) for m in meshes], cam16, H, W)
    out = np.array(np.broadcast_to(np.asarray(frame, dtype=np.uint8), (H, W, 3)))
    v = np.zeros((H, W, 3))
    for r, c in zip(*np.nonzero(owner >= 0)):
        _, f, col = meshes[owner[r, c]]
        v[r, c] = mesh_value(bary[r, c], np.asarray(col)[np.asarray(f).reshape(-1, 3)[face[r, c]]])
        out[r, c] = blend(v[r, c], out[r, c], opacity)
    if keypoints is not None and len(keypoints):
        out = paint_keypoints(out, keypoints, kp_rgb, kp_conf, radius)
    return out, owner, v


# ------------------------------------------------------------------------------------------------ the base scene of the GPU tests
H, W, M = 37, 53, 3
CAM = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, 60.0, 60.0, W / 2.0 + 0.3, H / 2.0 + 0.2]
KP_CONF, KP_RADIUS = 0.3, 3
KP_RGB = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], dtype=np.uint8)


def base_scene(seed=11):
    """5 records into 3 images: image 0 = two interpenetrating spheres and a copy of the first sphere's nearest triangle at
    identical vertices (an exact cross-record depth tie); image 1 = a sphere partly off screen and a 3-face mesh: one triangle
    spanning the image (the queue), one face behind z_clip, one zero-area face; image 2 = nothing.
    -> dict(meshes [(verts, faces, colors)], image_of, frames (M, H, W, 3), keypoints (M, 6, 3), tie_face)"""
    rs = np.random.RandomState(seed)
    va, f = icosphere((-0.12, 0.02, 3.0), 0.5)
    vb, _ = icosphere((0.27, 0.05, 3.1), 0.5)
    vc, _ = icosphere((1.3, 0.3, 3.0), 0.5)
    tie = int(np.argmin(va[f].mean(1)[:, 2]))                                  # A's triangle nearest to the camera
    vt, ft = va[f[tie]].copy(), np.array([[0, 1, 2]], dtype=np.int32)
    vm = np.array([[-10, -8, 5], [10, -8, 5], [0, 12, 5],                      # spans the image, behind the sphere
                   [0.1, 0.1, -1], [0.3, 0.1, 2], [0.1, 0.3, 2],               # one vertex behind the camera: dropped, not clipped
                   [-0.5, -0.2, 2], [-0.3, -0.2, 2], [-0.1, -0.2, 2]], dtype=np.float32)      # collinear: zero area
    fm = np.arange(9, dtype=np.int32).reshape(3, 3)
    col = lambda n: rs.uniform(0.05, 0.95, (n, 3)).astype(np.float32)          # away from the clamp: see test_colours
    meshes = [(va, f, col(42)), (vb, f, col(42)), (vt, ft, col(3)), (vc, f, col(42)), (vm, fm, col(9))]
    frames = rs.randint(0, 256, (M, H, W, 3)).astype(np.uint8)
    kp = np.zeros((M, 6, 3), dtype=np.float32)
    kp[0] = [[0.4, 0.7, 0.9],                 # at a corner
             [W - 1.5, 20.2, 0.8],            # straddling the right border
             [W + 10.0, -9.0, 0.9],           # fully outside
             [np.nan, 12.0, 0.9],             # NaN x
             [30.0, 8.0, 0.2],                # confidence below the threshold
             [W - 3.6, 21.9, 0.7]]            # overlaps keypoint 1 with another colour: the higher index wins
    kp[1] = kp[0, ::-1] * [0.5, 0.9, 1.0]
    kp[2, :, :2] = rs.uniform(0, 30, (6, 2))
    kp[2, :, 2] = [0.9, 0.1, 0.5, 0.3, 0.31, 0.0]
    return dict(meshes=meshes, image_of=[0, 0, 0, 1, 1], frames=frames, keypoints=kp, tie_face=tie)
