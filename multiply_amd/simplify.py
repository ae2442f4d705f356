"""Mesh simplification on the device: vertex clustering with quadric-optimal representatives (Lindstrom 2000, "Out-of-core
simplification of large polygonal models").  The algorithm is stated once, in float64, in
tests/mesh_simplify_reference.py; csrc/simplify.hip holds the kernels (everything that reads a coordinate), and this module the
sorts, `unique` calls and prefix sums between them, as mesh.marching_cubes does for its welding.

    verts', faces', info = simplify_mesh(verts, faces, cell=0.01)            # a cell size
    verts', faces', info = simplify_mesh(verts, faces, target_faces=50_000)  # or a face count, met to 2 % by bisecting the cell
    n_cells, n_live = cluster_counts(verts, faces, 0.01)

The result is a function of the input alone: the same bits on every run (no float atomics; every sum has a fixed order)."""
import math

import numpy as np
import torch

from . import hip

LAM = 1e-3
MAX_PASSES, COUNT_TOL = 16, 0.02
_INDEX_END = 1 << hip.SIMPLIFY_BITS


def _mesh_args(verts, faces):
    """(verts (V,3) float32, faces (F,3) int32) contiguous on the device; ValueError for what cannot be simplified"""
    if not isinstance(verts, torch.Tensor):
        verts = torch.as_tensor(np.asarray(verts, np.float32))
    if not isinstance(faces, torch.Tensor):
        faces = torch.as_tensor(np.asarray(faces, np.int64))
    if not verts.is_cuda:
        hip.require_device()
        verts = verts.cuda()
    faces = faces.to(verts.device)
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 and faces.numel():
        raise ValueError(f"verts must be (V, 3) and faces (F, 3), got {tuple(verts.shape)} and {tuple(faces.shape)}")
    if faces.dtype.is_floating_point or faces.dtype == torch.bool:
        raise ValueError(f"faces must be integers, got {faces.dtype}")
    verts = verts.detach().float().contiguous()
    faces = faces.reshape(-1, 3)
    V, F = verts.shape[0], faces.shape[0]
    if 3 * F >= 2 ** 31 or V >= 2 ** 31:
        raise ValueError("the mesh is too large: 3 F and V must stay below 2^31")
    if F and (V == 0 or int(faces.min()) < 0 or int(faces.max()) >= V):
        raise ValueError(f"a face refers to a vertex outside [0, {V})")
    return verts, faces.to(torch.int32).contiguous()


def _box(verts):
    """(min (3,), max (3,)) float32 numpy; ValueError for a non-finite vertex (min and max carry a NaN or an infinity along)"""
    if verts.shape[0] == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    box = torch.stack([verts.amin(0), verts.amax(0)]).cpu().numpy()
    if not np.isfinite(box).all():
        raise ValueError("a vertex is not finite")
    return box[0], box[1]


def _cell_args(h, lo, box):
    """(h, inv_h as fp32 values, lo (3,) float32); ValueError when an index of the bounding box does not fit"""
    h32 = np.float32(h)
    if not (np.isfinite(h32) and h32 > 0):
        raise ValueError(f"cell size must be positive and finite, got {h}")
    with np.errstate(over="ignore"):
        inv_h = np.float32(1.0) / h32
    lo = np.asarray(lo, np.float32).reshape(3)
    if not (np.isfinite(inv_h) and np.isfinite(lo).all()):
        raise ValueError(f"cell size {h} or origin {lo} is out of range")
    # the kernel's arithmetic on the box: fp32 subtraction and multiplication are monotone, so the box bounds every index
    q = np.floor((np.stack(box).astype(np.float32) - lo[None]) * inv_h)
    if not np.isfinite(q).all() or q.min() < 0 or q.max() >= _INDEX_END:
        raise ValueError(f"a cell index does not fit in {hip.SIMPLIFY_BITS} bits: cell {h} is too small for this mesh or origin")
    return float(h32), float(inv_h), lo


def _origin(origin, box):
    if origin is None:
        return box[0]
    if isinstance(origin, torch.Tensor):
        origin = origin.detach().cpu().numpy()
    return np.asarray(origin, np.float32).reshape(3)


def _live_count(verts, faces, h, lo, box):
    h, inv_h, lo = _cell_args(h, lo, box)
    key = hip.simplify_keys(verts, lo, inv_h)
    return key, hip.simplify_count(faces, key)


def cluster_counts(verts, faces, cell, origin=None):
    """(occupied cells, faces whose corners lie in three different cells) for cell size `cell`: what a simplification at that size
    starts from"""
    verts, faces = _mesh_args(verts, faces)
    box = _box(verts)
    key, live = _live_count(verts, faces, cell, _origin(origin, box), box)
    return int(torch.unique(key).shape[0]), int(live.sum())


def bisection_ends(box):
    """(h_lo, h_hi): shortest bounding-box side / 2^20 -- the longest side / 2^20 where the shortest is zero or its cell would not
    fit the index bits along the longest side -- and the longest side"""
    side = box[1].astype(np.float64) - box[0].astype(np.float64)
    longest, shortest = float(side.max()), float(side.min())
    if not longest > 0:
        raise ValueError("the mesh has no extent")
    h_lo = shortest / 2 ** 20
    if not (h_lo > 0 and longest / h_lo < _INDEX_END - 2):
        h_lo = longest / 2 ** 20
    return h_lo, longest


def _pick_cell(verts, faces, target, lo, box):
    """the cell size whose non-collapsed face count is within COUNT_TOL of target: geometric bisection, at most MAX_PASSES count
    passes (two launches and a sum each); the counts are integers, so the walk is the reference's"""
    if not target >= 1:
        raise ValueError(f"target_faces must be at least 1, got {target}")
    h_lo, h_hi = bisection_ends(box)
    passes = 0
    while True:
        h = float(np.float32(math.sqrt(h_lo * h_hi)))
        _, live = _live_count(verts, faces, h, lo, box)
        n, passes = int(live.sum()), passes + 1
        if abs(n - target) <= COUNT_TOL * target or passes == MAX_PASSES:
            return h, passes
        if n > target:
            h_lo = h
        else:
            h_hi = h


def _starts(counts):
    out = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=out[1:])
    return out


def _tick(stages, name):
    """tools/simplify_bench.py: an event at the END of stage `name` (nothing unless a list is passed)"""
    if stages is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        stages.append((name, e))


def simplify_mesh(verts, faces, cell=None, target_faces=None, attrs=None, origin=None, lam=LAM, stages=None):
    """Simplify the mesh verts (V,3), faces (F,3) (tensors or arrays; the work is on the device): every vertex falls into a cubic
    cell of size `cell` from `origin` (default: the per-axis minimum), each occupied cell gets ONE vertex at the minimum of its
    faces' plane quadrics, regularised towards the mean of its vertices by `lam` and clamped to the cell, faces with two corners in
    one cell drop out, and of faces that became equal (in either winding) the first stays.  Exactly one of `cell` and
    `target_faces` (then the cell is bisected until the number of surviving faces, before de-duplication, is within 2 % of it).
    attrs (V,K): per-vertex rows averaged per cell.

    Returns verts' (V',3) float32, faces' (F',3) int64 on the device and info: cell, origin, n_cells, n_collapsed, n_duplicate,
    n_unreferenced (cells no surviving face uses; they are dropped), passes (count passes of the bisection), attrs (V',K).
    stages: a list that receives (stage name, event recorded at its end) pairs, for timing."""
    if (cell is None) == (target_faces is None):
        raise ValueError("give exactly one of cell and target_faces")
    if not (lam > 0 and math.isfinite(lam)):
        raise ValueError(f"lam must be positive and finite, got {lam}")
    verts, faces = _mesh_args(verts, faces)
    V, F, dev = verts.shape[0], faces.shape[0], verts.device
    if attrs is not None:
        if not isinstance(attrs, torch.Tensor):
            attrs = torch.as_tensor(np.asarray(attrs, np.float32))
        if attrs.dim() != 2 or attrs.shape[0] != V:
            raise ValueError(f"attrs must be (V, K) = ({V}, K), got {tuple(attrs.shape)}")
        attrs = attrs.detach().to(dev).float().contiguous()
    box = _box(verts)
    lo = _origin(origin, box)
    passes = 0
    _tick(stages, "start")
    if cell is None:
        cell, passes = _pick_cell(verts, faces, target_faces, lo, box)
        _tick(stages, "bisection: count passes")
    h, inv_h, lo = _cell_args(cell, lo, box)
    info = dict(cell=h, origin=lo.copy(), n_cells=0, n_collapsed=F, n_duplicate=0, n_unreferenced=0, passes=passes)
    empty = (torch.zeros(0, 3, dtype=torch.float32, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev))
    if attrs is not None:
        info["attrs"] = torch.zeros(0, attrs.shape[1], dtype=torch.float32, device=dev)
    if V == 0:
        return empty + (info,)

    # 1. cells: key per vertex, cell id = rank among the occupied keys
    key = hip.simplify_keys(verts, lo, inv_h)
    _tick(stages, "keys")
    keys, cell_id, counts = torch.unique(key, return_inverse=True, return_counts=True)
    C = keys.shape[0]
    _tick(stages, "torch: unique of the keys")
    info["n_cells"] = C
    # 4. faces: ids, live flag, the unordered triple; equal triples side by side in ascending face order; the first is kept
    tri, key_lo, key_hi, live = hip.simplify_faces(faces, cell_id.to(torch.int32))
    n_live = int(live.sum()) if F else 0
    _tick(stages, "faces: ids, flags, triples")
    info["n_collapsed"] = F - n_live
    if n_live == 0:
        info["n_unreferenced"] = C
        return empty + (info,)
    by_hi = torch.sort(key_hi, stable=True).indices
    order = by_hi[torch.sort(key_lo[by_hi], stable=True).indices]
    _tick(stages, "torch: two stable sorts of the triples")
    keep = hip.simplify_first(order, key_lo, key_hi, live)
    kept = torch.nonzero(keep).reshape(-1)
    info["n_duplicate"] = n_live - kept.shape[0]
    out_faces = tri[kept].long()
    _tick(stages, "first of each triple, kept faces")
    # 2. + 3. the cells' sorted segments, quadrics, representatives
    pair_order = torch.sort(tri.reshape(-1), stable=True).indices
    pair_start = _starts(torch.bincount(tri.reshape(-1), minlength=C))
    vert_order = torch.sort(cell_id, stable=True).indices
    vert_start = _starts(counts)
    _tick(stages, "torch: sorts and prefix sums of the segments")
    pos = hip.simplify_quadrics(verts, faces, keys, pair_order, pair_start, vert_order, vert_start, lo, h, lam)
    _tick(stages, "quadrics and representatives")
    # 5. compaction: the cells a kept face refers to, in key order
    used = torch.zeros(C, dtype=torch.bool, device=dev)
    used[out_faces.reshape(-1)] = True
    new_id = torch.cumsum(used, 0) - 1
    info["n_unreferenced"] = C - int(new_id[-1]) - 1
    if attrs is not None:
        info["attrs"] = hip.simplify_attr_mean(attrs, vert_order, vert_start)[used]
    out = pos[used], new_id[out_faces], info
    _tick(stages, "torch: compaction" + (" and attribute means" if attrs is not None else ""))
    return out
