"""Quadric vertex clustering (Lindstrom 2000) in float64, numpy only: the statement of the algorithm that csrc/simplify.hip and
multiply_amd/simplify.py reproduce.

  1. cell     ijk = floor((v - lo) * inv_h) per axis IN FLOAT32 (inv_h = 1.0f / h, one subtraction and one multiplication, each
              rounded to nearest): the cell of a vertex is a matter of bits, not of a tolerance.  key = i << 42 | j << 21 | k,
              cell id = rank of the key among the occupied keys.
  2. quadric  per cell, in double, relative to the cell's centre c = lo + (ijk + 0.5) h: for every face and each of its three
              corners the corner's cell receives n n^T and n (n . (p0 - c)), n = (p1 - p0) x (p2 - p0) unnormalised; beside it the
              count and the mean of the cell's own vertices, relative to c.
  3. point    (A + l I) x = b + l mean with l = lam trace(A) / 3; x = mean where trace(A) == 0; clamped to the cell; c + x rounded
              once to float32.
  4. faces    corners -> cell ids; faces whose ids are not distinct drop out; of the faces with one unordered id triple the one with
              the lowest index stays, with its own winding; the kept faces stay in their order.
  5. compact  the cells some kept face refers to, in ascending key order.
  6. attrs    per cell the plain mean of its vertices' rows, summed in double, rounded once.
  7. target   a geometric bisection of h on the number of non-collapsed faces (pick_cell).
Every product and sum below is written out term by term, in the order the kernels use, so that a zero-area face gives n = 0
exactly on both sides (the mean branch of step 3 is taken on trace(A) == 0, a bit-exact condition)."""
import numpy as np

BITS = 21
LAM = 1e-3


def origin_of(verts):
    return np.asarray(verts, np.float32).reshape(-1, 3).min(0)


def cell_indices(verts, h, lo):
    """(V,3) int64 cell indices; ValueError for a non-finite vertex or an index outside [0, 2^21)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    h32, lo32 = np.float32(h), np.asarray(lo, np.float32).reshape(3)
    if not (np.isfinite(h32) and h32 > 0):
        raise ValueError(f"cell size must be positive and finite, got {h}")
    if not np.isfinite(v).all():
        raise ValueError("a vertex is not finite")
    inv_h = np.float32(1.0) / h32
    q = np.floor((v - lo32[None]) * inv_h)                    # float32 - float32 and float32 * float32: rounded to nearest each
    if v.shape[0] and (not np.isfinite(q).all() or q.min() < 0 or q.max() >= 2 ** BITS):
        raise ValueError(f"a cell index does not fit in {BITS} bits: cell {h} is too small for this mesh or origin")
    return q.astype(np.int64)


def pack(ijk):
    return (ijk[:, 0] << (2 * BITS)) | (ijk[:, 1] << BITS) | ijk[:, 2]


def unpack(key):
    m = (1 << BITS) - 1
    return np.stack([key >> (2 * BITS), (key >> BITS) & m, key & m], 1)


def cell_ids(verts, h, lo=None):
    """(occupied keys ascending (C,), cell id per vertex (V,))"""
    lo = origin_of(verts) if lo is None else lo
    uniq, cell = np.unique(pack(cell_indices(verts, h, lo)), return_inverse=True)
    return uniq, cell.reshape(-1)


def cluster_counts(verts, faces, h, lo=None):
    """(occupied cells, faces whose three corners lie in three different cells)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    uniq, cell = cell_ids(verts, h, lo)
    fc = cell[faces]
    live = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    return int(uniq.shape[0]), int(live.sum())


def bisection_ends(verts):
    """(h_lo, h_hi) of the bisection: shortest bounding-box side / 2^20 (the longest side / 2^20 where that cell would not fit
    the 21 index bits along the longest side, or the shortest side is zero) and the longest side"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    side = v.max(0).astype(np.float64) - v.min(0).astype(np.float64)
    longest, shortest = float(side.max()), float(side.min())
    if not longest > 0:
        raise ValueError("the mesh has no extent")
    h_lo = shortest / 2 ** 20
    if not (h_lo > 0 and longest / h_lo < 2 ** BITS - 2):
        h_lo = longest / 2 ** 20
    return h_lo, longest


def pick_cell(verts, faces, target, lo=None, max_passes=16, tol=0.02):
    """h (a float32 value) by geometric bisection on the non-collapsed face count, and the walk [(h, n_live)]"""
    if not target >= 1:
        raise ValueError("target_faces must be at least 1")
    h_lo, h_hi = bisection_ends(verts)
    walk = []
    for _ in range(max_passes):
        h = float(np.float32(np.sqrt(h_lo * h_hi)))
        _, live = cluster_counts(verts, faces, h, lo)
        walk.append((h, live))
        if abs(live - target) <= tol * target:
            break
        if live > target:
            h_lo = h
        else:
            h_hi = h
    return walk[-1][0], walk


def simplify(verts, faces, h, lo=None, lam=LAM, attrs=None):
    """dict: verts (V',3) float32, verts64 (the same before the final rounding), faces (F',3) int64, cell (V,) cell id per input
    vertex, keys (C,), used (V',) cell id per output vertex, info (the counts), attrs / attrs64 when given, and per OUTPUT vertex
    what the rounding bound needs: seg (contributions of its cell), n_verts, reach (largest |p0 - c| of a contribution plus |x|
    before the clamp)"""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    lo32 = origin_of(v32) if lo is None else np.asarray(lo, np.float32).reshape(3)
    h64 = float(np.float32(h))
    keys, cell = cell_ids(v32, h, lo32)
    C, F = keys.shape[0], faces.shape[0]
    v = v32.astype(np.float64)
    centre = lo32.astype(np.float64)[None] + (unpack(keys).astype(np.float64) + 0.5) * h64
    count = np.bincount(cell, minlength=C).astype(np.float64)
    mean = np.zeros((C, 3))
    np.add.at(mean, cell, v - centre[cell])
    mean /= np.maximum(count, 1.0)[:, None]

    fc = cell[faces] if F else np.zeros((0, 3), np.int64)
    p0 = v[faces[:, 0]]
    a, b = v[faces[:, 1]] - p0, v[faces[:, 2]] - p0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    # the 3 F contributions in the order of the pair index 3 f + corner
    pc = fc.reshape(-1)
    nn = np.repeat(n, 3, 0)
    d = np.repeat(p0, 3, 0) - centre[pc]
    nd = nn[:, 0] * d[:, 0] + nn[:, 1] * d[:, 1] + nn[:, 2] * d[:, 2]
    A, rhs = np.zeros((C, 6)), np.zeros((C, 3))
    np.add.at(A, pc, np.stack([nn[:, 0] * nn[:, 0], nn[:, 0] * nn[:, 1], nn[:, 0] * nn[:, 2], nn[:, 1] * nn[:, 1], nn[:, 1] * nn[:, 2],
                               nn[:, 2] * nn[:, 2]], 1))
    np.add.at(rhs, pc, nn * nd[:, None])
    seg = np.bincount(pc, minlength=C)
    far = np.zeros(C)
    np.maximum.at(far, pc, np.sqrt((d * d).sum(1)))

    trace = A[:, 0] + A[:, 3] + A[:, 5]
    l = lam * trace / 3.0
    M = np.zeros((C, 3, 3))
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2] = A.T
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    x = mean.copy()
    solve = trace > 0
    if solve.any():
        Ms = M[solve] + l[solve, None, None] * np.eye(3)[None]
        x[solve] = np.linalg.solve(Ms, (rhs[solve] + l[solve, None] * mean[solve])[:, :, None])[:, :, 0]
    reach = far + np.sqrt((x * x).sum(1))
    half = 0.5 * h64
    pos64 = centre + np.clip(x, -half, half)

    live = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    live_idx = np.nonzero(live)[0]
    if live_idx.shape[0]:
        _, first = np.unique(np.sort(fc[live_idx], 1), axis=0, return_index=True)      # first = lowest index of each triple
        kept = np.sort(live_idx[first])
    else:
        kept = live_idx
    used = np.unique(fc[kept])
    remap = np.full(C, -1, np.int64)
    remap[used] = np.arange(used.shape[0])
    out = dict(verts64=pos64[used], verts=pos64[used].astype(np.float32), faces=remap[fc[kept]].reshape(-1, 3), cell=cell, keys=keys,
               used=used, seg=seg[used], n_verts=count[used].astype(np.int64), reach=reach[used], mean64=(centre + mean)[used],
               info=dict(cell=h64, origin=lo32.copy(), n_cells=int(C), n_collapsed=int(F - live_idx.shape[0]),
                         n_duplicate=int(live_idx.shape[0] - kept.shape[0]), n_unreferenced=int(C - used.shape[0]), passes=0))
    if attrs is not None:
        at = np.asarray(attrs, np.float32).reshape(v32.shape[0], -1).astype(np.float64)
        s = np.zeros((C, at.shape[1]))
        np.add.at(s, cell, at)
        out["attrs64"] = (s / np.maximum(count, 1.0)[:, None])[used]
        out["attrs"] = out["attrs64"].astype(np.float32)
    return out


def simplify_to(verts, faces, target, lo=None, lam=LAM, attrs=None):
    h, walk = pick_cell(verts, faces, target, lo)
    out = simplify(verts, faces, h, lo, lam, attrs)
    out["info"]["passes"] = len(walk)
    out["walk"] = walk
    return out


# ------------------------------------------------------------------------------------------------ measures of a result
def is_watertight(faces):
    """every directed edge once, and its reverse present"""
    f = np.asarray(faces, np.int64)
    if f.shape[0] == 0:
        return False
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    m = int(f.max()) + 1
    key, rev = e[:, 0] * m + e[:, 1], e[:, 1] * m + e[:, 0]
    return bool(np.unique(key).shape[0] == key.shape[0] and np.array_equal(np.sort(key), np.sort(rev)))


def volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def point_triangle_distance(p, tri):
    """distances (P,) from points p (P,3) to the nearest of the triangles tri (F,3,3), float64 (Ericson's closest point)"""
    p = np.asarray(p, np.float64)[:, None]
    a, b, c = (np.asarray(tri, np.float64)[None, :, k] for k in range(3))
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        vv, ww = vb / den, vc / den
        q = a + ab * vv[..., None] + ac * ww[..., None]                                   # interior
        t = d1 / (d1 - d3)
        q = np.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * t[..., None], q)
        t = d2 / (d2 - d6)
        q = np.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * t[..., None], q)
        t = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        q = np.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * t[..., None], q)
    q = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c + 0 * ab, q)
    q = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b + 0 * ab, q)
    q = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a + 0 * ab, q)
    return np.nanmin(np.sqrt(((p - q) ** 2).sum(-1)), axis=1)               # (a zero-area triangle's interior branch is NaN)
