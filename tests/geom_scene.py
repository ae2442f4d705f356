"""The scene of the geometry front-end tests (tests/test_geom_oracle64_cpu.py, test_rays_gpu.py, test_warp_samples_gpu.py): one
posed synthetic body, a pinhole camera with skew that looks at it from the side, a row-major jittered pixel grid and the depth
tables of the warp tests.  Everything here is host-side fp32 INPUT data; the CPU test asserts on it, by the float64 reference
alone, the conditions the GPU tests rely on (how many rays graze a box, how many points sit on the outlier radius, ...)."""
import numpy as np
import torch

R_FULL = 3 * 1024 + 7          # rays of the cull tests: three full scan blocks and a ragged one
RADIUS = 3.0                   # bounding sphere of the scene (the camera is inside)
NEAR = 0.0
COLS = 64
K_WARP = 700                   # hit rays of the warp tests
NS, ZSTRIDE = 64, 640          # sampler form: 64 samples per ray in rows of 640
S_SHADE = 65                   # shading form: 65 samples (9 runs of 8, the last one ragged) in rows of 66
Z_LO, Z_HI = 1.6, 3.4          # the depths bracket the body (about 2.5 from the camera) by most of a metre on either side


def body_params():
    from multiply_amd.synthetic import make_scene
    return torch.tensor(make_scene(2, seed=0, H=16, W=16)["smpl_params"][0, 0], dtype=torch.float32)      # [86]


def camera():
    """K (4,4) with unequal focal lengths, an off-centre principal point and skew; pose (4,4) camera-to-world, looking at the body"""
    K = np.eye(4, dtype=np.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1] = 64.0, 66.0, 32.5, 31.25, 3.0
    eye, target, up = np.array([0.45, 0.05, -2.4]), np.array([-0.3, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4, dtype=np.float64)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return torch.tensor(K, dtype=torch.float32), torch.tensor(pose, dtype=torch.float32)


def pixels(n=R_FULL, seed=3):
    """n pixels of a COLS-wide jittered grid over the 64 x 64 image, row after row (consecutive rays are neighbours)"""
    rng = np.random.RandomState(seed)
    rows = -(-n // COLS)
    i = np.arange(n)
    u = ((i % COLS) + 0.5 + rng.uniform(-0.4, 0.4, n)) * (64.0 / COLS)
    v = ((i // COLS) + 0.5 + rng.uniform(-0.4, 0.4, n)) * (64.0 / rows)
    return torch.tensor(np.stack([u, v], 1), dtype=torch.float32)


def outside_camera_pixels(n=257, seed=5):
    """pixels of a wide image for the far-root test with the sphere radius 1: the camera is outside that sphere, the rays towards
    the image's rim miss it"""
    rng = np.random.RandomState(seed)
    return torch.tensor(rng.uniform(-40.0, 104.0, (n, 2)), dtype=torch.float32)


FAR_GRAZE = 1e-2      # rays with |discriminant| below this are left out of the far-root comparison (sqrt is ill-conditioned at 0)


def pca_box(verts, inflate=1.2):
    """a principal-axes box of the vertices like mp_obb's, on the host in float64 (the CPU test's stand-in for the device box)"""
    v = np.asarray(verts, dtype=np.float64)
    m = v.mean(0)
    _, ax = np.linalg.eigh(np.cov((v - m).T))
    ax = ax.T[::-1]
    p = (v - m) @ ax.T
    lo, hi = p.min(0), p.max(0)
    centre = m + ((lo + hi) * 0.5) @ ax
    return torch.tensor(np.concatenate([centre, ax.reshape(-1), (hi - lo) * 0.5 * inflate]), dtype=torch.float32)


def axis_box(verts, part="body"):
    """hand-made axis-aligned boxes (identity axes): around the whole body, or around its top 0.3 only"""
    v = np.asarray(verts, dtype=np.float64)
    lo, hi = v.min(0), v.max(0)
    if part == "top":
        a = int(np.argmax(hi - lo))                  # the body's long axis
        lo[a] = hi[a] - 0.3
    return torch.tensor(np.concatenate([(lo + hi) * 0.5, np.eye(3).reshape(-1), (hi - lo) * 0.5 + 0.02]), dtype=torch.float32)


def everything_box():
    return torch.tensor([0, 0, 0] + list(np.eye(3).reshape(-1)) + [100.0, 100.0, 100.0], dtype=torch.float32)


def nothing_box():
    return torch.tensor([0, 50.0, 0] + list(np.eye(3).reshape(-1)) + [0.1, 0.1, 0.1], dtype=torch.float32)


def spot_box(cam, dirs, ray=200, depth=2.5, half=0.08):
    """a small box on ray `ray`: only rays of the pixel rows around that ray's meet it, whole convergence groups miss it"""
    c = np.asarray(cam, dtype=np.float64) + depth * np.asarray(dirs[ray], dtype=np.float64)
    return torch.tensor(np.concatenate([c, np.eye(3).reshape(-1), [half] * 3]), dtype=torch.float32)


def parallel_dirs(dirs):
    """the scene's directions with one component of every 7th / 11th ray set to exactly 0 (and renormalised): rays parallel to a
    face pair of an axis-aligned box"""
    d = torch.as_tensor(dirs).clone().float()
    d[0::7, 1] = 0.0
    d[3::11, 0] = 0.0
    return torch.nn.functional.normalize(d, dim=1)


def sampler_depths(k=K_WARP, n_s=NS, stride=ZSTRIDE, seed=11):
    """[k][stride]: n_s ascending jittered depths per row; the columns behind n_s hold NaN (never read)"""
    rng = np.random.RandomState(seed)
    z = np.full((k, stride), np.nan, dtype=np.float32)
    step = (Z_HI - Z_LO) / n_s
    z[:, :n_s] = Z_LO + (np.arange(n_s)[None] + rng.uniform(0.05, 0.95, (k, n_s))) * step
    return torch.from_numpy(z)


def shade_depths(k=K_WARP, s=S_SHADE, seed=12):
    """[k][s + 1] strictly ascending depths (every interval at least 5 % of the mean step)"""
    return sampler_depths(k, s + 1, s + 1, seed)


def pick_rays(hit_ids, k=K_WARP):
    """k of the hit rays, evenly spread, ascending"""
    hit_ids = torch.as_tensor(hit_ids).long()
    sel = torch.linspace(0, hit_ids.numel() - 1, k).round().long()
    return hit_ids[sel]


def sample_points(cam, dirs_hit, z, n_s):
    """float64 positions of the implicit samples cam + z[k][s] d[k], [k * n_s][3], from the fp32 inputs"""
    p = cam.double()[None, None] + z[:, :n_s].double()[..., None] * dirs_hit.double()[:, None]
    return p.reshape(-1, 3)


# fp32 evaluation error of the kernels' nearest-vertex arithmetic, as a bound on the difference of two computed squared distances.
# A point is x = cam + t d evaluated in fp32 (a product and a sum, or one fused operation): each component is off by at most
# 2 u |x|_max, u = 2^-24, so the point by e_x <= 2 sqrt(3) u X with X = 4 (the scene lies within |x| < 4).  For a vertex at distance d
# the kernel computes fl(d^2) from three rounded subtractions f_i = (x_i - v_i)(1 + u), one rounded product and two fused
# multiply-adds: at most 5 roundings on any term, |fl(d^2) - d^2| <= 5 u d^2 (1 + O(u)) for the point it holds; against the float64
# point the squared distance moves by at most 2 d e_x + e_x^2.  Two candidates are compared, each with that error, hence the factor 2.
U32 = 2.0 ** -24
POINT_ERR = 2.0 * 3 ** 0.5 * U32 * 4.0


def d2_eval_bound(d2):
    return 2.0 * (5.0 * U32 * d2 * (1 + 1e-6) + 2.0 * d2.sqrt() * POINT_ERR + POINT_ERR ** 2)


# ---- the same scene on the device (GPU tests only) ------------------------------------------------------------------------------
_DEVICE_SCENE = {}


def ray_setup(uv, K, pose, radius):
    """mp_ray_setup on the first len(uv) pixels -> dirs [R][3], far [R] (device)"""
    import ctypes as C
    from multiply_amd import hip
    n = uv.shape[0]
    dirs = torch.full((n + 8, 3), -77.0, device="cuda")
    far = torch.full((n + 8,), -77.0, device="cuda")
    hip.lib().mp_ray_setup(uv.cuda().contiguous(), K.cuda().reshape(16).contiguous(), pose.cuda().reshape(16).contiguous(), n,
                           C.c_float(radius), dirs, far, hip.stream())
    torch.cuda.synchronize()
    assert (dirs[n:] == -77.0).all() and (far[n:] == -77.0).all()              # nothing written behind the last ray
    return dirs[:n].contiguous(), far[:n].contiguous()


def device_scene(smpl_tables):
    """the posed body (device SMPL server), its search tables and blend table, the camera's rays and the device's PCA box"""
    if "scene" in _DEVICE_SCENE:
        return _DEVICE_SCENE["scene"]
    from multiply_amd import hip
    from multiply_amd.smpl import SMPLServer, knn_cluster_perm
    prm = body_params().cuda()
    sv = SMPLServer(gender="male", betas=prm[76:].cpu().numpy(), smpl_tables=smpl_tables)
    out = sv(prm[0], prm[1:4], prm[4:76], prm[76:])
    verts, tfs = out["smpl_verts"][0].contiguous(), out["smpl_tfs"][0].reshape(24, 16).contiguous()
    verts_c = sv.verts_c[0].contiguous()
    perm = torch.from_numpy(knn_cluster_perm(verts_c.cpu().numpy())).cuda()
    vsorted, cbound = hip.knn_tables(verts, perm)
    vsorted_c, cbound_c = hip.knn_tables(verts_c, perm)
    skin_w = sv.tables.lbs_weights.contiguous()
    K, pose = camera()
    uv = pixels()
    dirs, far = ray_setup(uv, K, pose, RADIUS)
    obb = torch.zeros(16, device="cuda")
    hip.lib().mp_obb(verts, 1.2, obb, hip.stream())
    torch.cuda.synchronize()
    sc = dict(verts=verts, tfs=tfs, verts_c=verts_c, vsorted=vsorted, cbound=cbound, vsorted_c=vsorted_c, cbound_c=cbound_c,
              skin_w=skin_w, btab=hip.blend_table(skin_w, tfs), K=K, pose=pose, pose_d=pose.cuda().reshape(16).contiguous(),
              cam=pose[:3, 3].cuda(), uv=uv, dirs=dirs, far=far, obb=obb)
    _DEVICE_SCENE["scene"] = sc
    return sc


SENTINEL = -7


def ray_cull(sc, obb, n, group, dirs=None, near_beta=None, cbound="scene", far="scene"):
    """mp_ray_cull (near_beta None) or mp_ray_cull_near on the first n rays -> hit_index [n + 8] (pre-filled with SENTINEL), count,
    inv_index [n + 8] (pre-filled): host tensors.  scan_tmp is sized as the product sizes it (multiply.py)."""
    from multiply_amd import hip
    L = hip.lib()
    i32 = dict(dtype=torch.int32, device="cuda")
    hit = torch.full((n + 8,), SENTINEL, **i32)
    inv = torch.full((n + 8,), SENTINEL, **i32)
    count = torch.full((1,), SENTINEL, **i32)
    scan_tmp = torch.full((n + (n + 1023) // 1024 + 8,), SENTINEL, **i32)
    d = (sc["dirs"] if dirs is None else dirs)[:n].contiguous()
    obb = obb.cuda().contiguous()
    if near_beta is None:
        L.mp_ray_cull(d, sc["pose_d"], obb, n, group, hit, count, inv, scan_tmp, hip.stream())
    else:
        beta = torch.tensor([near_beta], dtype=torch.float32, device="cuda")
        L.mp_ray_cull_near(d, sc["pose_d"], obb, sc["cbound"] if cbound == "scene" else cbound,
                           sc["far"][:n].contiguous() if far == "scene" else far, beta, NEAR, n, group, hit, count, inv, scan_tmp,
                           hip.stream())
    torch.cuda.synchronize()
    assert (scan_tmp[n + (n + 1023) // 1024:] == SENTINEL).all()              # the scratch the header promises, and no more
    return hit.cpu().long(), int(count.item()), inv.cpu().long()
