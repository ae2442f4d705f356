"""TEST INFRASTRUCTURE (imported by tests/ only).  Float64 restatement of the geometry front end: camera rays and the far
root of the bounding sphere (rend_util.py:45-87, 131-147), the ray / box hit set with its per-group fallback and ordered
compaction (multiply.py:256-266), the nearest-vertex warp into canonical space (deformer.py:19-50) and the outlier override
(multiply.py:142-143).  Plain torch: every function takes fp32 or fp64 tensors on any device, computes in float64 and is the
yardstick of tests/test_rays_gpu.py and tests/test_warp_samples_gpu.py; tests/test_geom_oracle64_cpu.py pins it to the fp32
oracle (oracle/multiply_oracle.py) and to oracle/obb_oracle.py.  The one fp32 function is alpha4_fp32: the rule it restates
is "exactly 0 in fp32"."""
import numpy as np
import torch

OUTLIER_RADIUS = 0.1          # deformer.py:49


def _d(t):
    return torch.as_tensor(t).double()


def camera_rays64(uv, K, pose):
    """uv (R,2), K (4,4), pose (4,4) camera-to-world -> unit dirs (R,3), cam (3,): the pixel lifted to depth 1 with skew
    (rend_util.py:73-87), taken to world space, minus the camera centre, normalised (rend_util.py:45-70)"""
    uv, K, pose = _d(uv), _d(K).reshape(4, 4), _d(pose).reshape(4, 4)
    fx, fy, cx, cy, sk = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
    x, y = uv[:, 0], uv[:, 1]
    xl = (x - cx + cy * sk / fy - sk * y / fy) / fx
    yl = (y - cy) / fy
    local = torch.stack([xl, yl, torch.ones_like(xl)], 1)
    d = local @ pose[:3, :3].T                       # world point - camera centre
    n = d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return d / n, pose[:3, 3].clone()


def sphere_far64(cam, dirs, radius):
    """far root t of |cam + t d| = radius per ray, clamped at 0; 0 where the ray misses the sphere (negative discriminant).
    Also returns the discriminant, so that a caller can leave grazing rays (|under| ~ 0: the root is ill-conditioned) out."""
    cam, dirs = _d(cam), _d(dirs)
    b = (dirs * cam).sum(-1)
    under = b * b - ((cam * cam).sum(-1) - float(radius) ** 2)
    far = torch.where(under >= 0, (under.clamp_min(0).sqrt() - b).clamp_min(0), torch.zeros_like(b))
    return far, under


def ray_box64(cam, dirs, obb15):
    """slab test of the rays cam + t d, t >= 0, against the box obb15 = centre3, axes (3 rows), half extents3 -> (hit flags,
    signed margin): the margin of oracle/obb_oracle.py rays_hitting_box -- min(t_out - t_in, t_out), >= 0 = hit, ~0 = the ray
    grazes an edge of the box (or the box ends at the camera)"""
    cam, dirs, obb = _d(cam), _d(dirs), _d(obb15).reshape(-1)
    centre, axes, half = obb[0:3], obb[3:12].reshape(3, 3), obb[12:15]
    o = (cam - centre) @ axes.T
    d = dirs @ axes.T
    inf = torch.full_like(d, float("inf"))
    par = d.abs() < 1e-300
    ds = torch.where(par, torch.ones_like(d), d)
    t1, t2 = (-half - o) / ds, (half - o) / ds
    inside = (o.abs() <= half)[None].expand_as(d)
    tn = torch.where(par, torch.where(inside, -inf, inf), torch.minimum(t1, t2))
    tf = torch.where(par, torch.where(inside, inf, -inf), torch.maximum(t1, t2))
    t_in, t_out = tn.max(1).values, tf.min(1).values
    margin = torch.minimum(t_out - t_in, t_out)
    return margin >= 0, margin


def segment_vertex_distance64(cam, dirs, near, far, verts, chunk=512):
    """per ray: min over the vertices of the distance from the vertex to the segment {cam + t d : near <= t <= far}
    (dirs are unit vectors; far (R,))"""
    cam, dirs, far, verts = _d(cam), _d(dirs), _d(far), _d(verts)
    out = torch.empty(dirs.shape[0], dtype=torch.float64, device=dirs.device)
    e = verts - cam                                                   # (V,3)
    for s in range(0, dirs.shape[0], chunk):
        d, tf = dirs[s:s + chunk], far[s:s + chunk]
        t = torch.minimum(torch.maximum(d @ e.T, torch.full_like(tf, float(near))[:, None]), tf[:, None])   # (r,V)
        q = e[None] - t[..., None] * d[:, None]
        out[s:s + chunk] = (q * q).sum(-1).min(1).values.sqrt()
    return out


def group_fallback(flags, group_size):
    """multiply.py:262-263 per convergence group: a block of `group_size` consecutive rays (the last one partial; <= 0: one group
    for all rays) without any hit gets its first ray"""
    f = torch.as_tensor(flags).bool().clone()
    n = f.shape[0]
    g = n if group_size <= 0 else int(group_size)
    for g0 in range(0, n, g):
        if not bool(f[g0:g0 + g].any()):
            f[g0] = True
    return f


def compact(flags):
    """ordered compaction -> hit_index (ascending flagged ids), inv_index (position in hit_index, -1 elsewhere), count"""
    f = torch.as_tensor(flags).bool()
    hit = torch.nonzero(f).reshape(-1)
    inv = torch.full((f.shape[0],), -1, dtype=torch.int64, device=f.device)
    inv[hit] = torch.arange(hit.shape[0], device=f.device)
    return hit, inv, int(hit.shape[0])


def blend_table64(skin_w, tfs):
    """[V][3][4]: row r of vertex v = (I[r][0..2], c[r]) with T = sum_j skin_w[v][j] tfs[j], I = T[:3,:3]^-1, c = T[:3,3] / T[3,3];
    the inverse written out as the adjugate over the determinant (no library factorisation in the yardstick)"""
    w, tfs = _d(skin_w), _d(tfs).reshape(-1, 4, 4)
    T = torch.einsum("vj,jab->vab", w, tfs)
    M = T[:, :3, :3]
    cof = torch.stack([torch.cross(M[:, 1], M[:, 2], dim=-1), torch.cross(M[:, 2], M[:, 0], dim=-1),
                       torch.cross(M[:, 0], M[:, 1], dim=-1)], 1)             # rows = cofactors of the rows of M
    det = (M[:, 0] * cof[:, 0]).sum(-1)
    inv = cof.transpose(1, 2) / det[:, None, None]
    c = T[:, :3, 3] / T[:, 3, 3:4]
    return torch.cat([inv, c[:, :, None]], 2)


def nearest_vertex64(x, verts, chunk=4096):
    """brute force over all vertices -> (squared distance to the nearest vertex, its id: the LOWEST id at an exact tie, like an
    argmin over the original order (deformer.py:39), the gap: squared distance of the runner-up minus that of the nearest)"""
    x, verts = _d(x), _d(verts)
    n, dev = x.shape[0], x.device
    d2min = torch.empty(n, dtype=torch.float64, device=dev)
    gap = torch.empty(n, dtype=torch.float64, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    ids = torch.arange(verts.shape[0], device=dev)
    for s in range(0, n, chunk):
        p = x[s:s + chunk]
        d2 = ((p[:, None, :] - verts[None, :, :]) ** 2).sum(-1)
        m = d2.min(1, keepdim=True).values
        i = torch.where(d2 == m, ids[None], torch.full_like(ids, verts.shape[0])[None]).min(1).values
        d2.scatter_(1, i[:, None], float("inf"))
        d2min[s:s + chunk], idx[s:s + chunk], gap[s:s + chunk] = m[:, 0], i, d2.min(1).values - m[:, 0]
    return d2min, idx, gap


def outlier64(d2min):
    """deformer.py:41-49: sqrt(min(d2, 4)) > 0.1"""
    return d2min.clamp(max=4.0).sqrt() > OUTLIER_RADIUS


def warp64(x, nn, table64):
    """x_c = I (x - c) with the table row of the nearest vertex nn"""
    x = _d(x)
    t = table64[nn]
    return torch.einsum("pab,pb->pa", t[:, :, :3], x - t[:, :, 3])


def alpha4_fp32(beta, dt):
    """1 - exp(-(sigma(4) dt)) with the Laplace density sigma(s) = (1/beta)(0.5 + 0.5 sign(s) expm1(-|s|/beta)) (density.py:20-29),
    every operation in numpy float32 in the order the kernels use"""
    f = np.float32
    beta, dt = f(beta), np.asarray(dt, dtype=np.float32)
    sigma = (f(1.0) / beta) * (f(0.5) + f(0.5) * f(1.0) * np.expm1(-f(4.0) / beta, dtype=np.float32))
    return f(1.0) - np.exp(-(sigma * dt), dtype=np.float32)
