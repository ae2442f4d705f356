"""Canonical-mesh extraction on the device: the reference's `generate_mesh` (code/lib/utils/mesh.py:78-131) =
MISE lattice refinement (code/lib/libmise/mise.pyx, Cython/C++) around the network's zero level set, marching cubes
(skimage, third party) and the largest connected component (trimesh, third party).

MI355X-first: the finest lattice is dense in HBM and every MISE pass is a flat scan (csrc/mise.hip); the network is
queried with whole passes (up to millions of points) through the fused SDF kernel instead of 10 000-point batches; the
surface is extracted by a marching-cubes kernel pair (count, exclusive scan, emit) and welded by lattice-edge id.
`MISE` keeps the reference class's interface (resolution, query / update / to_dense), `generate_mesh` its signature.
The marching-cubes case table is DERIVED here (build_tri_table), not copied: crossing edges are joined face by face,
ambiguous faces always cut their inside corners off (the rule depends only on the face's own corners, so neighbouring
cubes agree and the surface has no holes), loops are fan-triangulated, winding = normals towards increasing values."""
import functools

import numpy as np
import torch

from . import hip

_CORNER = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])
_EDGE = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]   # = csrc/mise.hip


@functools.lru_cache(maxsize=None)
def build_tri_table():
    """[256][16] int32: per sign configuration (bit k = corner k below the level) the triangles as lattice-edge triples"""
    eid = {frozenset(e): i for i, e in enumerate(_EDGE)}
    mid = np.array([(_CORNER[a] + _CORNER[b]) / 2.0 for a, b in _EDGE])
    cube_faces = []
    for axis in range(3):
        for side in (0, 1):
            cs = [k for k in range(8) if _CORNER[k][axis] == side]
            order, rest = [cs[0]], set(cs[1:])
            while rest:                                   # walk the face's corners in cyclic order
                nxt = next(c for c in rest if np.abs(_CORNER[c] - _CORNER[order[-1]]).sum() == 1)
                order.append(nxt)
                rest.remove(nxt)
            normal = np.zeros(3)
            normal[axis] = 1.0 if side else -1.0
            cube_faces.append((order, normal))
    table = np.full((256, 16), -1, dtype=np.int32)
    for case in range(1, 255):
        inside = [(case >> k) & 1 for k in range(8)]
        succ = {}
        for order, normal in cube_faces:
            crossing = [eid[frozenset((order[i], order[(i + 1) % 4]))] for i in range(4)
                        if inside[order[i]] != inside[order[(i + 1) % 4]]]
            if len(crossing) == 2:
                segments = [tuple(crossing)]
            elif len(crossing) == 4:                      # ambiguous face: cut every inside corner off
                segments = [(eid[frozenset((order[(i - 1) % 4], order[i]))], eid[frozenset((order[i], order[(i + 1) % 4]))])
                            for i in range(4) if inside[order[i]]]
            else:
                segments = []
            for ea, eb in segments:                       # direct it: inside corners on the left, seen from outside the cube
                pa, pb = mid[ea], mid[eb]
                ci = min((c for c in order if inside[c]), key=lambda c: np.linalg.norm(_CORNER[c] - (pa + pb) / 2))
                if np.dot(np.cross(pb - pa, _CORNER[ci] - pa), normal) < 0:
                    ea, eb = eb, ea
                succ[ea] = eb
        seen, flat = set(), []
        for start in sorted(succ):
            if start in seen:
                continue
            loop, cur = [start], succ[start]
            seen.add(start)
            while cur != start:
                loop.append(cur)
                seen.add(cur)
                cur = succ[cur]
            for i in range(1, len(loop) - 1):             # fan; (0, i+1, i): normals towards the outside (larger values)
                flat += [loop[0], loop[i + 1], loop[i]]
        assert len(flat) <= 15
        table[case, :len(flat)] = flat
    return table


class MISE:
    """mise.pyx MISE(resolution_0, depth, threshold) on a dense device lattice."""

    def __init__(self, resolution_0, depth, threshold, device=None):
        hip.require_device()
        self.resolution_0, self.depth, self.threshold = int(resolution_0), int(depth), float(threshold)
        self.voxel_size_0 = 1 << self.depth
        self.resolution = self.resolution_0 * self.voxel_size_0
        self.device = torch.device("cuda") if device is None else device
        n = self.resolution + 1
        nvox = sum((self.resolution_0 << l) ** 3 for l in range(self.depth + 1))
        u8 = dict(dtype=torch.uint8, device=self.device)
        self.state = torch.empty(n, n, n, **u8)
        self.val = torch.zeros(n, n, n, dtype=torch.float32, device=self.device)
        self.vox = torch.zeros(nvox, **u8)
        self.pos, self.neg = torch.zeros(nvox, **u8), torch.zeros(nvox, **u8)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.n_split = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.n_queried = []
        hip.lib().mp_mise_init(self.resolution_0, self.depth, self.state, self.vox, hip.stream())

    def query(self):
        """lattice points (k, 3) int32 whose value is unknown (device tensor; order unspecified)"""
        L, n = hip.lib(), self.resolution + 1
        self.count.zero_()
        L.mp_mise_collect(n, self.state, self.count, 0, None, hip.stream())
        k = int(self.count.item())
        pts = torch.empty(max(k, 1), 3, dtype=torch.int32, device=self.device)
        if k:
            self.count.zero_()
            L.mp_mise_collect(n, self.state, self.count, k, pts, hip.stream())
        return pts[:k]

    def update(self, points, values):
        """store the values of queried points, then split every active leaf voxel (mise.pyx:80-97, 172-222)"""
        L, n = hip.lib(), self.resolution + 1
        pts = points.to(self.device).to(torch.int32).contiguous()
        vals = values.to(self.device).float().reshape(-1).contiguous()
        assert pts.shape[0] == vals.shape[0]
        L.mp_mise_scatter(n, pts, vals, pts.shape[0], self.state, self.val, hip.stream())
        self.pos.zero_()
        self.neg.zero_()
        L.mp_mise_refine(self.resolution_0, self.depth, self.threshold, self.state, self.val, self.vox, self.pos, self.neg,
                         self.n_split, hip.stream())
        self.n_queried.append(pts.shape[0])

    def to_dense(self):
        """(resolution+1)^3 fp32 values; lattice points that never became grid points inherit along x, then y, then z"""
        state, val = self.state.clone(), self.val.clone()
        hip.lib().mp_mise_fill(self.resolution + 1, state, val, hip.stream())
        return val


def marching_cubes(volume, level=0.0):
    """volume (n, n, n) fp32 device tensor -> vertices (V, 3) fp32 in lattice units, faces (F, 3) int64; shared vertices
    are welded (one vertex per crossed lattice edge), winding gives normals towards increasing values."""
    L = hip.lib()
    vol = volume.float().contiguous()
    n = vol.shape[0]
    assert vol.shape == (n, n, n) and n >= 2
    dev = vol.device
    table = torch.from_numpy(build_tri_table()).to(dev)
    counts = torch.empty((n - 1) ** 3, dtype=torch.int32, device=dev)
    L.mp_mc_count(vol, n, float(level), table, counts, hip.stream())
    ends = torch.cumsum(counts.long(), 0)
    T = int(ends[-1].item())
    if T == 0:
        return torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev)
    offsets = (ends - counts.long()).contiguous()
    corners = torch.empty(3 * T, 3, dtype=torch.float32, device=dev)
    edge_id = torch.empty(3 * T, dtype=torch.int64, device=dev)
    L.mp_mc_emit(vol, n, float(level), table, offsets, corners, edge_id, hip.stream())
    uniq, inverse = torch.unique(edge_id, return_inverse=True)
    verts = torch.empty(uniq.shape[0], 3, dtype=torch.float32, device=dev)
    verts[inverse] = corners                      # every corner of one lattice edge carries identical bits
    faces = inverse.reshape(T, 3)
    keep = (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 0] != faces[:, 2])
    return verts, faces[keep]


def largest_component(verts, faces):
    """the connected component with the largest surface area (mesh.py:119-129: trimesh split + max area), host side"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = faces.cpu().numpy()
    v = verts.cpu().numpy().astype(np.float64)
    if f.shape[0] == 0:
        return verts, faces
    nv = v.shape[0]
    rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    _, label = connected_components(coo_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(nv, nv)), directed=False)
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    flabel = label[f[:, 0]]
    best = np.argmax(np.bincount(flabel, weights=area))
    fk = f[flabel == best]
    used = np.unique(fk)
    remap = np.full(nv, -1, dtype=np.int64)
    remap[used] = np.arange(used.shape[0])
    return verts[torch.from_numpy(used).to(verts.device)], torch.from_numpy(remap[fk]).to(faces.device)


class ExtractedMesh:
    """What `generate_mesh` returns: the attribute surface of the `trimesh.Trimesh` the reference hands to its callers
    (lib/utils/mesh.py:117-131; multiply_model.py:311-314, 504-505, 845-847, 1180: `.vertices`, `.faces` as numpy arrays,
    `.split(only_watertight=False)`, `.area`, `.export(path)`), plus the device tensors the hot path re-uses
    (`vertices_t`, `faces_t`) and the extraction record (`value_grid`, `lattice_vertices`, `resolution`, `n_queried`).
    `mesh["vertices"]` / `mesh["faces"]` (device tensors) keep the dictionary access of the earlier interface."""

    def __init__(self, vertices_t, faces_t, **info):
        self.vertices_t, self.faces_t = vertices_t, faces_t
        self.vertices = vertices_t.detach().cpu().numpy()
        self.faces = faces_t.detach().cpu().numpy().astype(np.int64)
        self.info = info

    def __getitem__(self, k):
        if k == "vertices":
            return self.vertices_t
        if k == "faces":
            return self.faces_t
        return self.info[k]

    def __getattr__(self, k):          # value_grid, lattice_vertices, resolution, n_queried
        info = self.__dict__.get("info", {})
        if k in info:
            return info[k]
        raise AttributeError(k)

    @property
    def area(self):
        v, f = self.vertices.astype(np.float64), self.faces
        return float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())

    @property
    def is_watertight(self):
        """every edge is shared by exactly two faces, traversed once in each direction"""
        f = self.faces
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = e[:, 0] * (f.max() + 1) + e[:, 1]
        rev = e[:, 1] * (f.max() + 1) + e[:, 0]
        return bool(np.unique(key).shape[0] == key.shape[0] and np.array_equal(np.sort(key), np.sort(rev)))

    def split(self, only_watertight=False):
        """connected components (by shared vertices), each an ExtractedMesh -- what trimesh's split(only_watertight=False)
        gives the reference's largest-area selection (mesh.py:119-129)"""
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        f, nv = self.faces, self.vertices.shape[0]
        if f.shape[0] == 0:
            return []
        rows = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
        cols = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
        _, label = connected_components(coo_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(nv, nv)), directed=False)
        out = []
        for c in np.unique(label[f[:, 0]]):
            fk = f[label[f[:, 0]] == c]
            used = np.unique(fk)
            remap = np.full(nv, -1, dtype=np.int64)
            remap[used] = np.arange(used.shape[0])
            dev = self.vertices_t.device
            part = ExtractedMesh(self.vertices_t[torch.from_numpy(used).to(dev)], torch.from_numpy(remap[fk]).to(dev))
            if not only_watertight or part.is_watertight:
                out.append(part)
        return out

    def simplify(self, cell=None, target_faces=None):
        """the mesh reduced by quadric vertex clustering (multiply_amd/simplify.py): an ExtractedMesh whose record is that of
        simplify_mesh (cell, origin, n_cells, n_collapsed, n_duplicate, n_unreferenced, passes).  Exactly one of cell (the cluster
        size, in the mesh's unit) and target_faces."""
        from .simplify import simplify_mesh
        verts, faces, info = simplify_mesh(self.vertices_t, self.faces_t, cell=cell, target_faces=target_faces)
        return ExtractedMesh(verts, faces, **info)

    def export(self, path):
        """binary little-endian PLY (vertices float32, faces int32), the format the reference's callers write"""
        v, f = self.vertices.astype("<f4"), self.faces.astype("<i4")
        with open(path, "wb") as fh:
            fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\nproperty float x\nproperty float y\n"
                      f"property float z\nelement face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n").encode())
            fh.write(v.tobytes())
            rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
            rec["n"], rec["i"] = 3, f
            fh.write(rec.tobytes())
        return path


def lattice_to_world(points, resolution, gt_scale, gt_center, scale=1.1):
    """mesh.py:96-98 / :113-114, fp32 like the reference"""
    p = (points.float() / resolution - 0.5) * scale
    return p * gt_scale + gt_center


def generate_mesh(func, verts, level_set=0.0, res_init=32, res_up=3, point_batch=None):
    """mesh.py:78-131.  func(points (k,3) fp32 device) -> values (k,) / (k,1) or {'occ': ...}; verts (V,3): the box to
    search is their bounding cube, padded by 1.1.  Returns an ExtractedMesh (`.vertices` (V,3) / `.faces` (F,3) numpy like the
    reference's trimesh object, `.split()`, `.area`, `.export()`; device tensors and the extraction record beside them):
    the outward-facing triangles of the largest-area component (open where the level set leaves the box, like any
    marching-cubes surface).

    Triangulation: the case table is derived in build_tri_table (ambiguous faces separate their inside corners; no interior
    ambiguity test).  skimage's Lewiner tables (mesh.py:112, third party, absent here) resolve the ambiguous configurations by
    the asymptotic decider and so may connect a few saddle cubes differently: both surfaces pass through the same points of the
    same lattice edges (vertex SETS identical up to skimage's own vertex ordering) and are closed and consistently oriented; they
    differ, if at all, in how those points are joined inside ambiguous cubes.  Parity with skimage's face list is unpinned."""
    dev = torch.device("cuda")
    v = verts.detach().to(dev).float().reshape(-1, 3)
    lo, hi = v.min(dim=0).values, v.max(dim=0).values
    gt_center, gt_scale = (lo + hi) * 0.5, (hi - lo).max()
    ex = MISE(res_init, res_up, level_set, dev)
    pts = ex.query()
    while pts.shape[0] != 0:
        world = lattice_to_world(pts, ex.resolution, gt_scale, gt_center)
        chunks = [world] if not point_batch else torch.split(world, int(point_batch), dim=0)
        vals = []
        for c in chunks:
            out = func(c)
            out = out["occ"] if isinstance(out, dict) else out
            vals.append(out.detach().reshape(-1).float())
        ex.update(pts, torch.cat(vals))
        pts = ex.query()
    grid = ex.to_dense()
    mv, mf = marching_cubes(grid, level_set)
    mv, mf = largest_component(mv, mf)
    return ExtractedMesh(lattice_to_world(mv, ex.resolution, gt_scale, gt_center), mf, lattice_vertices=mv, value_grid=grid,
                         resolution=ex.resolution, n_queried=ex.n_queried)


def canonical_mesh(model, person, cond=None, res_init=32, res_up=2):
    """The trainer's refresh (multiply_model.py:503, 615: generate_mesh(query_oc, verts_c, point_batch=10000, res_up=2)):
    person's canonical zero level set through the fused SDF kernel.  cond = pose conditioning (69,), default zeros."""
    imp = model.foreground_implicit_network_list[person]
    dev = model.density.beta.device
    cond = torch.zeros(69, device=dev) if cond is None else cond.to(dev).float().reshape(-1)
    vc = model.smpl_server_list[person].verts_c[0]
    with torch.no_grad():
        return generate_mesh(lambda x: hip.implicit_sdf(imp, x.contiguous(), cond), vc, 0.0, res_init, res_up)


def refresh_canonical_meshes(model, conds=None, res_up=2):
    """what multiply_model.py:497-506 does every 20 epochs: re-extract every person's canonical mesh and re-assign
    mesh_v_cano_list / mesh_f_cano_list / mesh_face_vertices_list (read by the in / off-surface flags, multiply.py:153-167)"""
    vs, fs, fvs = [], [], []
    for p in range(model.num_person):
        m = canonical_mesh(model, p, None if conds is None else conds[p], res_up=res_up)
        vs.append(m["vertices"][None])
        fs.append(m["faces"])
        fvs.append(m["vertices"][m["faces"]][None])
    model.mesh_v_cano_list, model.mesh_f_cano_list, model.mesh_face_vertices_list = vs, fs, fvs
    return vs, fs
