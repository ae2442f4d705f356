"""Mesh-to-mesh metrics: how close a reconstructed mesh is to a ground-truth one.

The method this project restates is judged by Chamfer distance, point-to-surface distance, normal consistency and volumetric IoU
of its meshes against ground-truth scans, but the reference project ships no code for them -- there is nothing to match, so the
definitions below are the usual published ones (Mescheder et al., Occupancy Networks, CVPR 2019; Tatarchenko et al., What Do
Single-view 3D Reconstruction Networks Learn?, CVPR 2019), spelled out:

  samples            n points per mesh, area-uniform on its faces, with the normal of the face they lie on;
  directed distance  of a sample = the Euclidean distance to the closest point of the OTHER mesh's surface (exact, over all
                     faces: csrc/mesh_closest.hip brute force, or the face index of csrc/mesh_index.hip -- same bits);
  accuracy           mean directed distance of the prediction's samples to the ground truth;
  completeness       mean directed distance of the ground truth's samples to the prediction (also returned as p2s,
                     point-to-surface);
  chamfer            (accuracy + completeness) / 2;      chamfer_sq = the SUM of the two mean SQUARED distances;
  hausdorff          the larger of the two directed maxima (over the samples);
  normal_consistency the mean of the two directed means of |n . n'|, n the sample's normal and n' the normal of the closest
                     face; normal_consistency_signed the same without the absolute value (needs consistently oriented meshes);
  precision(t)       fraction of the prediction's samples nearer than t to the ground truth; recall(t) the converse;
  f_score(t)         2 P R / (P + R), 0 when P + R = 0;
  volume_iou         both meshes' insides (exact signed distance < 0) on a lattice of iou_resolution points per axis over the
                     joint bounding box -- the centres of its iou_resolution^3 cells, so that no point lies on the box itself:
                     |A and B| / |A or B| (0 for an empty union).  Closed meshes only.

Distances are multiplied by unit_scale (squared ones by its square); thresholds are given in the scaled unit.  Samples whose query
has no answer (non-finite coordinates) are left out of every mean and counted in n_left_out.  Everything heavy runs on the
device; this module imports without one."""
import numpy as np
import torch

from . import hip

_PLY_TYPES = {"char": "i1", "uchar": "u1", "short": "i2", "ushort": "u2", "int": "i4", "uint": "u4", "float": "f4", "double": "f8",
              "int8": "i1", "uint8": "u1", "int16": "i2", "uint16": "u2", "int32": "i4", "uint32": "u4", "float32": "f4",
              "float64": "f8"}


def load_ply(path):
    """vertices (V,3) float32 and faces (F,3) int64 of a triangle PLY, ASCII or binary little-endian (what ExtractedMesh.export
    writes); other vertex properties are skipped, other elements must come after the faces.  numpy only."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = raw.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in raw[:end].decode("ascii").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            elements[-1][2].append(w[1:])
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    if [e[0] for e in elements[:2]] != ["vertex", "face"]:
        raise ValueError(f"{path}: expected the elements vertex, face")
    (_, nv, vprops), (_, nf, fprops) = elements[:2]
    names = [p[-1] for p in vprops]
    if any(p[0] == "list" for p in vprops) or not all(k in names for k in "xyz"):
        raise ValueError(f"{path}: vertices need scalar properties x, y, z")
    if len(fprops) != 1 or fprops[0][0] != "list":
        raise ValueError(f"{path}: faces need exactly one list property")
    xyz = [names.index(k) for k in "xyz"]
    if fmt == "ascii":
        tok = raw[body:].split()
        k = len(vprops)
        verts = np.array(tok[:nv * k], dtype=np.float64).reshape(nv, k)[:, xyz]
        ft = np.array(tok[nv * k:nv * k + 4 * nf], dtype=np.float64).reshape(nf, 4)
        if nf and not (ft[:, 0] == 3).all():
            raise ValueError(f"{path}: only triangles are supported")
        faces = ft[:, 1:]
    else:
        vdt = np.dtype([(p[-1], "<" + _PLY_TYPES[p[0]]) for p in vprops])
        v = np.frombuffer(raw, dtype=vdt, count=nv, offset=body)
        verts = np.stack([v[k] for k in "xyz"], 1)
        fdt = np.dtype([("n", "<" + _PLY_TYPES[fprops[0][1]]), ("i", "<" + _PLY_TYPES[fprops[0][2]], (3,))])
        f = np.frombuffer(raw, dtype=fdt, count=nf, offset=body + nv * vdt.itemsize)
        if nf and not (f["n"] == 3).all():
            raise ValueError(f"{path}: only triangles are supported")
        faces = f["i"]
    return np.ascontiguousarray(verts, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.int64)


def as_mesh(mesh, device="cuda"):
    """(vertices (V,3) float32, faces (F,3) int64) device tensors of an ExtractedMesh, a (vertices, faces) pair of tensors or
    numpy arrays, or the path of a PLY file"""
    if isinstance(mesh, (str, bytes)) or hasattr(mesh, "__fspath__"):
        mesh = load_ply(mesh)
    elif hasattr(mesh, "vertices_t") and hasattr(mesh, "faces_t"):
        mesh = (mesh.vertices_t, mesh.faces_t)
    v, f = mesh
    v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().to(device).float().reshape(-1, 3).contiguous()
    f = torch.as_tensor(np.asarray(f) if not torch.is_tensor(f) else f).detach().to(device).long().reshape(-1, 3).contiguous()
    if f.shape[0] < 1:
        raise ValueError("a mesh needs at least one face")
    return v, f


def surface_samples(mesh, n, generator=None, uniforms=None):
    """n area-uniform points on the mesh: points (n,3), their faces' unit normals (n,3), face ids (n,) int32.  The uniforms
    (n,3) come from `generator` (a seeded DEVICE generator, as in smpl_init) unless given; face by the area CDF, barycentrics by
    the square-root map (mp_fit_area_cdf / mp_fit_sample with no volume points).  Zero-area faces are never drawn."""
    v, f = as_mesh(mesh)
    fv = v[f].contiguous()
    _, normal, cdf = hip.fit_area_cdf(fv)
    if uniforms is None:
        uniforms = torch.rand(int(n), 3, generator=generator, device=v.device)
    none = torch.empty(0, 3, dtype=torch.float32, device=v.device)
    return hip.fit_sample(fv, normal, cdf, uniforms.float().contiguous(), none, 0.0, none, None)


def directed(samples, target_mesh, index_mode="auto"):
    """d2 (n,), face (n,) int32, q (n,3) of the sample points (n,3) against target_mesh: squared distance to its closest face,
    that face and the closest point on it.  index_mode 'auto' | 'index' | 'brute' (hip.mesh_index_mode): 'auto' builds a face
    index from hip.MESH_INDEX_MIN_FACES faces on -- the closest query does not need a closed mesh.  Same bits either way."""
    v, f = as_mesh(target_mesh)
    fv = v[f].contiguous()
    pts = torch.as_tensor(samples).detach().to(v.device).float().reshape(-1, 3).contiguous()
    index = hip.MeshIndex(fv) if hip.mesh_index_wanted(index_mode, fv.shape[0], True) else None
    return hip.mesh_closest(pts, fv, index=index)


def _inside(pts, mesh, index_mode):
    v, f = mesh
    fv = v[f].contiguous()
    index = hip.MeshIndex(fv) if hip.mesh_index_wanted(index_mode, fv.shape[0], f) else None
    return torch.cat([hip.mesh_signed_distance(p.contiguous(), fv, index=index) < 0 for p in torch.split(pts, 1 << 22)])


def lattice_axis(lo, hi, R):
    """the R cell centres of [lo, hi], float32 (formed in float64, rounded once)"""
    return (np.float64(lo) + (np.arange(R) + 0.5) * ((np.float64(hi) - np.float64(lo)) / R)).astype(np.float32)


def volume_iou(pred, gt, resolution, index_mode="auto"):
    """|inside both| / |inside either| on resolution^3 lattice points, the cell centres of the joint bounding box.  The insides
    are the signs of mesh_signed_distance: fp32 distances with a ray-parity sign.  A lattice point ON a surface, or one whose +x
    ray runs exactly through a vertex or along an edge (an axis-aligned box whose faces are squares, sampled on its own diagonal),
    has no right answer there; meshes in general position do not meet the lattice that way, and the cell centres keep it off the
    bounding box, which the outermost faces always touch.  ValueError unless both meshes are closed."""
    pred, gt = as_mesh(pred), as_mesh(gt)
    for name, (v, f) in (("pred", pred), ("gt", gt)):
        if not hip.faces_closed(f):
            raise ValueError(f"volume_iou needs closed meshes: {name} is not (an edge is not shared by exactly two faces)")
    R = int(resolution)
    lo = torch.minimum(pred[0].min(0).values, gt[0].min(0).values).cpu().numpy()
    hi = torch.maximum(pred[0].max(0).values, gt[0].max(0).values).cpu().numpy()
    ax = [torch.from_numpy(lattice_axis(lo[k], hi[k], R)).to(pred[0].device) for k in range(3)]
    pts = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    a, b = _inside(pts, pred, index_mode), _inside(pts, gt, index_mode)
    union = int((a | b).sum())
    return float(int((a & b).sum()) / union) if union else 0.0


def _align(P, G, align, options, seed, index_mode):
    """the prediction (vertices, faces) carried into the ground truth's frame, and the `align` entry of mesh_metrics' result"""
    from . import registration as reg
    if isinstance(align, reg.Similarity):
        T, kind, info = align, "given", dict(rms=None, iterations=0, converged=None)
    elif isinstance(align, str) and align in reg.KINDS:
        opts = dict(seed=seed, index_mode=index_mode)
        opts.update(options or {})
        T, info = reg.register(P, G, kind=align, **opts)
        kind = align
    else:
        raise ValueError(f"align must be None, one of {reg.KINDS} or a registration.Similarity, got {align!r}")
    aligned = dict(kind=kind, scale=T.scale, matrix=T.matrix.tolist(), rms=info["rms"], iterations=info["iterations"],
                   converged=info["converged"])
    return (reg.transform_vertices(P[0], T), P[1]), aligned


def mesh_metrics(pred, gt, n_samples=100_000, thresholds=(), seed=0, unit_scale=1.0, iou_resolution=None, index_mode="auto",
                 details=None, align=None, align_options=None):
    """The metrics of the module's docstring between the meshes pred and gt (ExtractedMesh, (vertices, faces), or a PLY path) as
    a dict of floats (precision / recall / f_score: lists, one entry per threshold).  Both meshes are sampled with the SAME
    n_samples uniforms of a device generator seeded with `seed`, so a mesh's samples do not depend on which argument it is:
    swapping pred and gt swaps accuracy and completeness exactly.  details: a dict that receives the samples and the two queries
    (for tests and plots).  align: None (both meshes share a frame), 'rigid' / 'similarity' (registration.register of pred onto gt,
    with the keyword arguments in align_options) or a registration.Similarity; the prediction's vertices are transformed before
    sampling and before volume_iou, and the result gains align = {kind, scale, matrix, rms, iterations, converged}."""
    if align is not None:
        from . import registration as reg
        if not isinstance(align, reg.Similarity) and not (isinstance(align, str) and align in reg.KINDS):
            raise ValueError(f"align must be None, one of {reg.KINDS} or a registration.Similarity, got {align!r}")
    P, G = as_mesh(pred), as_mesh(gt)
    aligned = None
    if align is not None:
        P, aligned = _align(P, G, align, align_options, seed, index_mode)
    dev, s = P[0].device, float(unit_scale)
    if len(thresholds) > 8:
        raise ValueError("at most 8 thresholds")
    u = torch.rand(int(n_samples), 3, generator=torch.Generator(device=dev).manual_seed(int(seed)), device=dev)
    tau = [float(t) / s for t in thresholds]
    red = {}
    for name, src, dst in (("accuracy", P, G), ("completeness", G, P)):
        pts, nrm, fid = surface_samples(src, n_samples, uniforms=u)
        d2, face, q = directed(pts, dst, index_mode)
        fn = hip.fit_area_cdf(dst[0][dst[1]])[1]
        red[name] = hip.mesh_metric_reduce(d2, face, nrm, fn, tau)
        if details is not None:
            details[name] = dict(points=pts, normals=nrm, sample_face=fid, d2=d2, face=face, q=q)
    a, c = (red[k].cpu().tolist() for k in ("accuracy", "completeness"))
    T = len(tau)
    prec = [a[7 + k] / a[5] if a[5] else 0.0 for k in range(T)]
    rec = [c[7 + k] / c[5] if c[5] else 0.0 for k in range(T)]
    out = dict(accuracy=s * a[0], completeness=s * c[0], p2s=s * c[0], chamfer=s * (0.5 * (a[0] + c[0])),
               chamfer_sq=s * s * (a[1] + c[1]), hausdorff=s * max(a[2], c[2]), normal_consistency=0.5 * (a[4] + c[4]),
               normal_consistency_signed=0.5 * (a[3] + c[3]), thresholds=[float(t) for t in thresholds], precision=prec,
               recall=rec, f_score=[2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)],
               n_samples=int(n_samples), n_left_out=int(a[6] + c[6]))
    if iou_resolution:
        out["volume_iou"] = volume_iou(P, G, iou_resolution, index_mode)
    if aligned is not None:
        out["align"] = aligned
    return out
