"""Meshes of the simplification tests (test_mesh_simplify_*.py): numpy float32 vertices (V,3), int64 faces (F,3).  The spheres
and the planar grid are those of tests/mesh_metrics_shapes.py."""
import numpy as np

from tests.mesh_metrics_shapes import icosphere, quad_grid, squashed  # noqa: F401  (re-exported)

BOX_LO, BOX_HI = np.array([-0.5, -0.4, -0.3]), np.array([0.5, 0.6, 0.7])


def box_corners():
    return np.array([[x, y, z] for x in (BOX_LO[0], BOX_HI[0]) for y in (BOX_LO[1], BOX_HI[1]) for z in (BOX_LO[2], BOX_HI[2])])


def tessellated_box(k=24):
    """the box [BOX_LO, BOX_HI] with k x k quads per side, welded along edges and corners, outward winding:
    6 k^2 + 2 vertices and 12 k^2 faces (k = 24: 3 458 and 6 912)"""
    ids, lattice, faces = {}, [], []

    def vid(p):
        if p not in ids:
            ids[p] = len(lattice)
            lattice.append(p)
        return ids[p]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, k):
            for i in range(k):
                for j in range(k):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:                              # (u, w, axis) is right-handed: this order faces +axis
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    v = BOX_LO[None] + (BOX_HI - BOX_LO)[None] * np.array(lattice, float) / k
    return v.astype(np.float32), np.array(faces, np.int64)


def two_sided_sheet():
    """quad_grid(8, 0.25) and, 0.01 above it, the same grid with reversed winding: 162 vertices, 256 faces"""
    v0, f0 = quad_grid(8, 0.25)
    v1, f1 = quad_grid(8, 0.26)
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1[:, ::-1] + v0.shape[0]]).astype(np.int64)


def lattice_sheet(h=0.125, k=9):
    """a k x k x 2 lattice of vertices at exact multiples of h from its first vertex (which sits at (-1, 0.5, 2): exact in float32),
    so that every vertex lies ON a cell face; two layers of quads"""
    base = np.array([-1.0, 0.5, 2.0])
    idx = np.array([[i, j, l] for l in range(2) for i in range(k) for j in range(k)])
    v = (base[None] + idx * h).astype(np.float32)
    f = []
    for l in range(2):
        o = l * k * k
        for i in range(k - 1):
            for j in range(k - 1):
                a, b, c, d = o + i * k + j, o + (i + 1) * k + j, o + (i + 1) * k + j + 1, o + i * k + j + 1
                f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int64)
