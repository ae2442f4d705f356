"""Meshes and point sets of the closest-face and mesh-metric tests (test_mesh_closest_gpu.py, test_mesh_metrics_*.py): numpy
float32 vertices (V,3) and int64 faces (F,3).  The sphere and point-set recipes are those of test_mesh_index_gpu.py, restated."""
import numpy as np
import torch


def icosphere(n=3, radius=0.5, base=8):
    """an octahedron (base 8: 8 * 4^n faces) or icosahedron (base 20: 20 * 4^n faces) subdivided n times onto the sphere"""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    if base == 20:
        t = (1 + 5 ** 0.5) / 2
        v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float) / (1 + t * t) ** 0.5
        f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                      [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                      [9, 8, 1]])
    for _ in range(n):
        cache, vs, nf = {}, list(v), []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (vs[a] + vs[b]) / 2
                cache[k] = len(vs)
                vs.append(m / np.linalg.norm(m))
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(vs), np.array(nf)
    return (v * radius).astype(np.float32), f.astype(np.int64)


def squashed(n, radius=0.5, base=20):
    """the squashed, offset sphere: not symmetric, not centred"""
    v, f = icosphere(n, radius, base)
    return (v * np.array([1.0, 1.4, 0.7], np.float32) + np.array([0.03, -0.02, 0.05], np.float32)).astype(np.float32), f


def box(lo, hi):
    """the closed 12-face box [lo, hi], outward normals"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    v = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]])
    return v.astype(np.float32), f.astype(np.int64)


def cube():
    return box([-0.5, -0.4, -0.3], [0.5, 0.6, 0.7])


def unit_square(z=0.0):
    """the unit square [0,1]^2 in the plane z, two faces, normal +z"""
    v = np.array([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int64)


def quad_grid(k=2, z=0.25):
    """a planar k x k quad grid (2 k^2 faces): zero extent along z"""
    xs = np.linspace(-0.5, 0.5, k + 1)
    v = np.array([[x, y, z] for x in xs for y in xs], np.float32)
    n = k + 1
    f = [[i * n + j, (i + 1) * n + j, i * n + j + 1] for i in range(k) for j in range(k)]
    f += [[(i + 1) * n + j, (i + 1) * n + j + 1, i * n + j + 1] for i in range(k) for j in range(k)]
    return v, np.array(f, np.int64)


def point_sets(v, f, seed):
    """{name: (n,3) float32 tensor} around the mesh (v, f): inside / near / far, and points ON vertices, edge midpoints and
    centroids (where faces tie by construction)"""
    v, f = torch.as_tensor(v), torch.as_tensor(f)
    g = torch.Generator().manual_seed(seed)
    fv = v[f]
    lo, hi = v.min(0).values, v.max(0).values
    ctr, ext = (lo + hi) / 2, (hi - lo).max()
    pick = lambda t, k: t[torch.randperm(t.shape[0], generator=g)[:k]]
    sets = {}
    mix = (torch.rand(900, 3, generator=g) - 0.5) * 2.0
    mix[:120] *= 0.2
    mix[120:240] = mix[120:240] * 0.1 + torch.tensor([0.9, 0.9, 0.9])
    sets["mix"] = mix * (ext / 1.4) + ctr
    near = pick(fv.mean(1), 600)
    sets["near"] = near + 2e-3 * ext * torch.randn(near.shape, generator=g)
    d = torch.randn(300, 3, generator=g)
    sets["far"] = ctr + 10.0 * ext * d / d.norm(dim=1, keepdim=True)
    sets["on vertices"] = pick(v, 400)
    e = pick(torch.cat([fv[:, [0, 1]], fv[:, [1, 2]], fv[:, [2, 0]]]), 400)
    sets["on edge midpoints"] = (e[:, 0] + e[:, 1]) / 2
    sets["on centroids"] = pick(fv.mean(1), 400)
    return {k: p.float().contiguous() for k, p in sets.items()}
