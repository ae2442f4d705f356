"""Refining SMPL fits to 2D keypoints on the device: the `refine` mode of the reference's preprocessing
(preprocessing/preprocessing_multiple_trace.py:360-527, preprocessing/loss.py), whose output is the `smpl_params` every dataset reads.

For every frame and person the reference runs 150 Adam steps on betas, pose and translation against

    L = w_2d sum_k c_k sum_{u,v} rho^2 r^2 / (r^2 + rho^2)  +  w_t ( w_p mean_{24x6}(d rot6D^2) + mean_3(d transl^2) )

r = detected - projected keypoint (GMoF, rho = 100), c_k = (conf_k joint_weight_k)^2 / (2 K) (joints_2d_loss: a mean over K x 2 of
the squared weights), rot6D = the first two columns of each joint's rotation, the temporal target = the previous frame's refined
pose and translation held constant; w_2d = 1e-2, w_t = 6, w_p = 5 (loss.py:11-15, :476).  The objective needs the body only at the
24 joints and at the few SUPPORT VERTICES the keypoints are regressed from, so csrc/keypoint_fit.hip evaluates it, its adjoint and
the whole Adam loop in one launch, one workgroup per person-frame (mp_kp_fit; mp_kp_objective is one evaluation).

  KeypointMap          keypoint k = sum_m a_km src[i_km], src = [24 posed joints ; S support vertices], validated CSR.  A row may be
                       a kinematic joint, one vertex, or a sparse regressor row over vertices.  coco25() / coco17() are the
                       reference's smpl_to_pose(model_type='smpl') mappings into its 54 joints = 24 kinematic + 21 selector
                       vertices + the 9 rows of J_regressor_extra.npy (which the user supplies: extra_regressor (9, 6890)).
  keypoint_weights     c of confidences: threshold, the map's joint weights (coco25 ignores joints 1, 9, 12), 1 / (2 K_set).
  keypoint_objective   terms, gradient and projections of N rows in one launch;  project_keypoints: the projections alone.
  refine_frame         the P persons of one frame in one launch (all Adam steps inside it).
  refine_sequence      the reference's frame loop: start values, temporal targets, tracked pairs, copied frames.

Parameters are rows of 85 = [transl 3, thetas 72, betas 10] (pack_params / split_params); scale is 1 and the transforms absolute,
as in the reference's fit.  Not built: the spline interpolation of missing frames (interpolate_frames copies, as the loop does),
person matching, the distance gate between the two keypoint sets (the overlay images: overlay.py).  This module imports without a device."""
import warnings

import numpy as np
import torch

from . import hip

N_PARAMS, MAX_K, MAX_S = 85, 64, 256                      # = include/multiply_hip.h MP_KP_PARAMS, MP_KP_MAX_K, MP_KP_MAX_S
N_VERTS, N_JOINTS = 6890, 24
REFERENCE_WEIGHTS = dict(rho=100.0, w_2d=1e-2, w_t=6.0, w_p=5.0)          # loss.py:9-15, preprocessing_multiple_trace.py:476
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8)                             # torch.optim.Adam(betas=(0.9, 0.999))
# the 21 vertices smplx's VertexJointSelector appends to the 24 joints of a SMPL body (vertex_ids['smplh']): nose, reye, leye,
# rear, lear, LBigToe, LSmallToe, LHeel, RBigToe, RSmallToe, RHeel, then the left and the right hand's finger tips
SELECTOR_VERTS = (332, 6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787,
                  2746, 2319, 2445, 2556, 2673, 6191, 5782, 5905, 6016, 6133)
N_EXTRA = 9                                                               # rows of J_regressor_extra.npy: joints 45 .. 53
COCO25_SMPL54 = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34)
COCO17_SMPL54 = (24, 26, 25, 28, 27, 16, 17, 18, 19, 20, 21, 46, 45, 4, 5, 7, 8)
COCO25_IGNORED = (1, 9, 12)                                               # joints_2d_loss: joints_to_ign


def pack_params(pose, trans, shape):
    """(..., 72), (..., 3), (..., 10) -> (..., 85) = [transl, thetas, betas]"""
    return torch.cat([trans, pose, shape], -1)


def split_params(p):
    """(..., 85) -> pose (..., 72), trans (..., 3), shape (..., 10)"""
    return p[..., 3:75], p[..., 0:3], p[..., 75:85]


class KeypointMap:
    """A validated CSR map from [24 joints ; S support vertices] to K keypoints.  ptr (K + 1,), idx / w (nnz,), support (S,) = the
    mesh vertex ids of the support vertices (unique); joint_weights (K,) multiplies the confidences (0 = ignored keypoint)."""

    def __init__(self, ptr, idx, w, support=(), joint_weights=None, name="custom"):
        ptr, idx = np.asarray(ptr), np.asarray(idx)
        w, support = np.asarray(w, np.float64), np.asarray(support)
        if ptr.ndim != 1 or ptr.shape[0] < 2 or ptr.dtype.kind not in "iu":
            raise ValueError(f"ptr: expected (K + 1,) integers with K >= 1, got {ptr.shape} {ptr.dtype}")
        K = ptr.shape[0] - 1
        if K > MAX_K:
            raise ValueError(f"ptr: {K} keypoints exceed the kernel's cap of {MAX_K} (MP_KP_MAX_K)")
        if ptr[0] != 0 or (np.diff(ptr) < 0).any():
            raise ValueError(f"ptr: expected a non-decreasing row pointer that starts at 0, got {ptr.tolist()}")
        if idx.ndim != 1 or idx.shape[0] != ptr[-1] or w.shape != idx.shape or (idx.size and idx.dtype.kind not in "iu"):
            raise ValueError(f"idx / w: expected ({int(ptr[-1])},) integers and floats, got {idx.shape} {idx.dtype} and {w.shape}")
        if support.ndim != 1 or (support.size and support.dtype.kind not in "iu"):
            raise ValueError(f"support: expected (S,) integer vertex ids, got {support.shape} {support.dtype}")
        S = support.shape[0]
        if S > MAX_S:
            raise ValueError(f"support: {S} support vertices exceed the kernel's cap of {MAX_S} (MP_KP_MAX_S)")
        if S and (support.min() < 0 or support.max() >= N_VERTS or np.unique(support).size != S):
            raise ValueError(f"support: expected unique vertex ids in [0, {N_VERTS}), got [{support.min()}, {support.max()}], "
                             f"{np.unique(support).size} unique of {S}")
        if idx.size and (idx.min() < 0 or idx.max() >= N_JOINTS + S):
            raise ValueError(f"idx: sources must lie in [0, {N_JOINTS + S}), got [{idx.min()}, {idx.max()}]")
        if not np.isfinite(w).all():
            raise ValueError("w: the map's weights must be finite")
        jw = np.ones(K) if joint_weights is None else np.asarray(joint_weights, np.float64)
        if jw.shape != (K,) or not np.isfinite(jw).all():
            raise ValueError(f"joint_weights: expected ({K},) finite, got {jw.shape}")
        self.ptr, self.idx, self.w = ptr.astype(np.int32), idx.astype(np.int32), w.astype(np.float32)
        self.support, self.joint_weights, self.name = support.astype(np.int64), jw, name
        self.sets = [(0, K)]          # keypoint ranges that are one detector's set each (their own K_set)
        self.notes = []

    K = property(lambda self: self.ptr.shape[0] - 1)
    S = property(lambda self: self.support.shape[0])

    # ---- constructors
    @classmethod
    def from_rows(cls, rows, joint_weights=None, name="custom"):
        """rows: one per keypoint, each ('joint', j) | ('vertex', v) | ('regressor', vertex ids, weights) | ('empty',)"""
        support, entries = {}, []
        for r in rows:
            kind = r[0]
            if kind == "joint":
                j = int(r[1])
                if not 0 <= j < N_JOINTS:
                    raise ValueError(f"joint id {j} outside [0, {N_JOINTS})")
                entries.append([(j, 1.0)])
            elif kind == "vertex":
                entries.append([(("v", int(r[1])), 1.0)])
            elif kind == "regressor":
                ids, ws = np.asarray(r[1]).reshape(-1), np.asarray(r[2], np.float64).reshape(-1)
                if ids.shape != ws.shape:
                    raise ValueError(f"regressor row: {ids.shape} vertex ids against {ws.shape} weights")
                entries.append([(("v", int(i)), float(a)) for i, a in zip(ids, ws)])
            elif kind == "empty":
                entries.append([])
            else:
                raise ValueError(f"unknown row kind {kind!r}")
        verts = sorted({s[1] for e in entries for s, _ in e if isinstance(s, tuple)})
        for v in verts:
            if not 0 <= v < N_VERTS:
                raise ValueError(f"vertex id {v} outside [0, {N_VERTS})")
        support = {v: N_JOINTS + i for i, v in enumerate(verts)}
        ptr, idx, w = [0], [], []
        for e in entries:
            for s, a in e:
                idx.append(support[s[1]] if isinstance(s, tuple) else s)
                w.append(a)
            ptr.append(len(idx))
        return cls(np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(w), np.asarray(verts, np.int64), joint_weights, name)

    @classmethod
    def from_joints(cls, ids, **kw):
        return cls.from_rows([("joint", j) for j in ids], **kw)

    @classmethod
    def from_vertices(cls, ids, **kw):
        return cls.from_rows([("vertex", v) for v in ids], **kw)

    @staticmethod
    def regressor_rows(regressor):
        """dense (R, 6890) -> the rows for from_rows, the non-zero entries of each"""
        reg = np.asarray(regressor, np.float64)
        if reg.ndim != 2 or reg.shape[1] != N_VERTS:
            raise ValueError(f"regressor: expected (R, {N_VERTS}), got {reg.shape}")
        return [("regressor", np.nonzero(r)[0], r[np.nonzero(r)[0]]) for r in reg]

    @classmethod
    def from_regressor(cls, regressor, **kw):
        return cls.from_rows(cls.regressor_rows(regressor), **kw)

    @classmethod
    def from_smpl54(cls, indices, extra_regressor=None, joint_weights=None, name="smpl54"):
        """indices into the reference's 54 joints: 0-23 kinematic, 24-44 the selector vertices, 45-53 the rows of extra_regressor
        (9, 6890).  Without it those rows are empty, their joint weight is 0, and a warning says so."""
        extra = None
        if extra_regressor is not None:
            extra = np.asarray(extra_regressor, np.float64)
            if extra.shape != (N_EXTRA, N_VERTS):
                raise ValueError(f"extra_regressor: expected ({N_EXTRA}, {N_VERTS}) (J_regressor_extra.npy), got {extra.shape}")
            extra = cls.regressor_rows(extra)
        rows, missing = [], []
        jw = np.ones(len(indices)) if joint_weights is None else np.array(joint_weights, np.float64)
        for k, i in enumerate(indices):
            i = int(i)
            if 0 <= i < N_JOINTS:
                rows.append(("joint", i))
            elif i < N_JOINTS + len(SELECTOR_VERTS):
                rows.append(("vertex", SELECTOR_VERTS[i - N_JOINTS]))
            elif i < N_JOINTS + len(SELECTOR_VERTS) + N_EXTRA:
                if extra is None:
                    rows.append(("empty",))
                    jw[k] = 0.0
                    missing.append(k)
                else:
                    rows.append(extra[i - N_JOINTS - len(SELECTOR_VERTS)])
            else:
                raise ValueError(f"joint index {i} outside the reference's 54 joints")
        m = cls.from_rows(rows, jw, name)
        if missing:
            note = (f"{name}: keypoints {missing} are rows of J_regressor_extra.npy, which was not given (extra_regressor=None): "
                    f"they get zero weight and take no part in the fit")
            m.notes.append(note)
            warnings.warn(note)
        return m

    @classmethod
    def coco25(cls, extra_regressor=None):
        """smpl_to_pose(model_type='smpl', openpose_format='coco25'): OpenPose's 25 body keypoints; 1, 9, 12 are ignored"""
        jw = np.ones(25)
        jw[list(COCO25_IGNORED)] = 0.0
        return cls.from_smpl54(COCO25_SMPL54, extra_regressor, jw, "coco25")

    @classmethod
    def coco17(cls, extra_regressor=None):
        """smpl_to_pose(model_type='smpl', openpose_format='coco17'): ViTPose's 17 keypoints; the hips are extra-regressor rows"""
        return cls.from_smpl54(COCO17_SMPL54, extra_regressor, None, "coco17")

    def concat(self, other):
        """self's keypoints followed by other's, each keeping its own K_set (the reference's second keypoint set)"""
        rows = self.rows() + other.rows()
        m = KeypointMap.from_rows(rows, np.concatenate([self.joint_weights, other.joint_weights]), f"{self.name}+{other.name}")
        m.sets = list(self.sets) + [(a + self.K, b + self.K) for a, b in other.sets]
        m.notes = self.notes + other.notes
        return m

    # ---- views
    def rows(self):
        out = []
        for k in range(self.K):
            a, b = self.ptr[k], self.ptr[k + 1]
            idx, w = self.idx[a:b], self.w[a:b]
            if b == a:
                out.append(("empty",))
            elif b - a == 1 and idx[0] < N_JOINTS and w[0] == 1.0:
                out.append(("joint", int(idx[0])))
            elif b - a == 1 and w[0] == 1.0:
                out.append(("vertex", int(self.support[idx[0] - N_JOINTS])))
            elif (idx >= N_JOINTS).all():
                out.append(("regressor", self.support[idx - N_JOINTS], w.astype(np.float64)))
            else:
                raise ValueError(f"keypoint {k} mixes joints and vertices: build the concatenation from CSR arrays instead")
        return out

    def row_kinds(self):
        return [r[0] for r in self.rows()]

    def dense(self):
        """(K, 24 + S) float64"""
        M = np.zeros((self.K, N_JOINTS + self.S))
        for k in range(self.K):
            for m in range(self.ptr[k], self.ptr[k + 1]):
                M[k, self.idx[m]] += self.w[m]
        return M

    def transposed(self):
        """the same matrix by source: tptr (24 + S + 1,), tk, tw (nnz,), keypoints ascending within a source"""
        n = N_JOINTS + self.S
        k_of = np.repeat(np.arange(self.K), np.diff(self.ptr))
        order = np.lexsort((k_of, self.idx))
        tptr = np.zeros(n + 1, np.int32)
        np.cumsum(np.bincount(self.idx, minlength=n), out=tptr[1:])
        return tptr, k_of[order].astype(np.int32), self.w[order].astype(np.float32)

    def pack(self, servers):
        """the support pack of one SMPLServer (or a list: one table set per entry) on its device, built once with torch indexing"""
        return SupportPack(self, servers)


class SupportPack:
    """The tables mp_kp_* read: per table set j_template (24, 3), j_shapedirs (24, 3, 10), sv_template (S, 3), s_shapedirs
    (S, 3, 10), s_posedirs (207, 3 S), s_weights (S, 24), stacked over the sets; the CSR map and its transpose; parents."""

    def __init__(self, kmap, servers):
        servers = list(servers) if isinstance(servers, (list, tuple)) else [servers]
        if not servers:
            raise ValueError("servers: expected at least one SMPLServer")
        self.kmap, self.n_tables = kmap, len(servers)
        t0 = servers[0].tables
        dev = self.device = t0.v_template.device
        sv = torch.from_numpy(kmap.support).to(dev)
        S = kmap.S
        stack = lambda f: torch.stack([f(s.tables) for s in servers]).contiguous()
        self.j_template = stack(lambda t: t.j_regressor @ t.v_template)
        self.j_shapedirs = stack(lambda t: t.j_shapedirs)
        self.sv_template = stack(lambda t: t.v_template[sv])
        self.s_shapedirs = stack(lambda t: t.shapedirs[sv])
        self.s_posedirs = stack(lambda t: t.posedirs.view(207, N_VERTS, 3)[:, sv].reshape(207, 3 * S))
        self.s_weights = stack(lambda t: t.lbs_weights[sv])
        self.parents = t0.parents
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.map_ptr, self.map_idx, self.map_w = up(kmap.ptr), up(kmap.idx), up(kmap.w)
        self.tmap_ptr, self.tmap_k, self.tmap_w = (up(a) for a in kmap.transposed())
        if kmap.idx.size == 0:         # (an all-empty map: keep the pointers non-NULL)
            self.map_idx, self.tmap_k = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
            self.map_w, self.tmap_w = (torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(2))

    def table_args(self, row_table):
        """the table and map arguments of mp_kp_objective / mp_kp_fit, in the header's order (for raw calls)"""
        return (self.parents, self.j_template, self.j_shapedirs, self.sv_template, self.s_shapedirs, self.s_posedirs, self.s_weights,
                self.n_tables, row_table, self.map_ptr, self.map_idx, self.map_w, self.tmap_ptr, self.tmap_k, self.tmap_w,
                self.kmap.S, self.kmap.K)


# ------------------------------------------------------------------------------------------------ host-side preparation
def keypoint_weights(conf, kmap, conf_threshold=0.6):
    """c (..., K) = (conf_k joint_weight_k)^2 / (2 K_set) with confidences below the threshold set to 0 (joints_2d_loss: the mean
    over K_set x 2 of the squared weights times the robust residuals).  conf_threshold: one value, or one per set of the map."""
    conf = torch.as_tensor(conf)
    if conf.dim() < 1 or conf.shape[-1] != kmap.K or not conf.dtype.is_floating_point:
        raise ValueError(f"conf: expected floating-point (..., {kmap.K}), got {tuple(conf.shape)} {conf.dtype}")
    thr = [float(conf_threshold)] * len(kmap.sets) if np.ndim(conf_threshold) == 0 else [float(x) for x in conf_threshold]
    if len(thr) != len(kmap.sets):
        raise ValueError(f"conf_threshold: expected one value or one per keypoint set ({len(kmap.sets)}), got {len(thr)}")
    jw = torch.as_tensor(kmap.joint_weights, dtype=conf.dtype, device=conf.device)
    out = torch.empty_like(conf)
    for (a, b), th in zip(kmap.sets, thr):
        cs = conf[..., a:b]
        cs = torch.where(cs < th, torch.zeros_like(cs), cs)
        out[..., a:b] = (cs * jw[a:b]) ** 2 / (2.0 * (b - a))
    return out


def camera_rows(camera, N, device=None, dtype=torch.float32):
    """camera -> (N, 16) rows [fx, fy, cx, cy, E (3, 4)].  camera: a dict with 'intrinsics' (3, 3) (or fx, fy, cx, cy) and an
    optional 'extrinsic' (3, 4) / (4, 4) (identity: the reference fits in camera space); or ready rows (16,) / (N, 16)."""
    if isinstance(camera, dict):
        if "intrinsics" in camera:
            Kc = np.asarray(camera["intrinsics"], np.float64)
            if Kc.shape[0] < 3 or Kc.shape[1] < 3:
                raise ValueError(f"camera['intrinsics']: expected (3, 3), got {Kc.shape}")
            fx, fy, cx, cy = Kc[0, 0], Kc[1, 1], Kc[0, 2], Kc[1, 2]
        else:
            fx, fy, cx, cy = (float(camera[k]) for k in ("fx", "fy", "cx", "cy"))
        E = np.asarray(camera.get("extrinsic", np.eye(4)[:3]) if camera.get("extrinsic") is not None else np.eye(4)[:3], np.float64)
        if E.shape not in ((3, 4), (4, 4)):
            raise ValueError(f"camera['extrinsic']: expected (3, 4) or (4, 4), got {E.shape}")
        row = torch.tensor(np.concatenate([[fx, fy, cx, cy], E[:3].reshape(-1)]), dtype=dtype)
        return row[None].expand(N, 16).contiguous().to(device)
    rows = torch.as_tensor(camera).detach().to(dtype)
    if rows.dim() == 1:
        rows = rows[None].expand(N, -1)
    if rows.shape != (N, 16):
        raise ValueError(f"camera: expected a dict or rows (16,) / ({N}, 16), got {tuple(rows.shape)}")
    return rows.contiguous().to(device)


def _rows(x, name, shape, dev):
    x = torch.as_tensor(x).detach()
    want = tuple(shape)
    if x.dim() != len(want) or any(w is not None and s != w for s, w in zip(x.shape, want)):
        raise ValueError(f"{name}: expected {tuple('N' if w is None else w for w in want)}, got {tuple(x.shape)}")
    if not x.dtype.is_floating_point:
        raise ValueError(f"{name}: expected a floating-point tensor, got {x.dtype} with shape {tuple(x.shape)}")
    return x.to(device=dev, dtype=torch.float32).contiguous()


def _pack_of(servers, kmap, pack):
    if pack is not None:
        if pack.kmap is not kmap:
            raise ValueError("pack: built for another KeypointMap")
        return pack
    return kmap.pack(servers)


def _row_table(row_server, N, pack):
    if row_server is None:
        if pack.n_tables == 1:
            return None
        if pack.n_tables != N:
            raise ValueError(f"row_server: {pack.n_tables} servers against {N} rows needs the server of every row")
        row_server = np.arange(N)
    rs = np.asarray(row_server)
    if rs.shape != (N,) or rs.dtype.kind not in "iu" or (N and (rs.min() < 0 or rs.max() >= pack.n_tables)):
        raise ValueError(f"row_server: expected ({N},) integers in [0, {pack.n_tables}), got {rs.shape} {rs.dtype}")
    return torch.from_numpy(rs.astype(np.int32)).to(pack.device)


def _weights(kw):
    w = dict(REFERENCE_WEIGHTS)
    bad = [k for k in kw if k not in w]
    if bad:
        raise ValueError(f"unknown loss weights {bad}: expected a subset of {sorted(w)}")
    w.update(kw)
    return w["rho"], w["w_2d"], w["w_t"], w["w_p"]


def _inputs(servers, params, targets, c, kmap, camera, prev, row_server, pack):
    pack = _pack_of(servers, kmap, pack)
    dev = pack.device
    params = _rows(params, "params", (None, N_PARAMS), dev)
    N = params.shape[0]
    targets = _rows(targets, "targets", (N, kmap.K, 2), dev)
    c = _rows(c, "c", (N, kmap.K), dev)
    prev = None if prev is None else _rows(prev, "prev", (N, 75), dev)
    return pack, params, targets, c, prev, camera_rows(camera, N, dev), _row_table(row_server, N, pack), N


# ------------------------------------------------------------------------------------------------ launches
def keypoint_objective(servers, params, targets, conf, kmap, camera, prev=None, conf_threshold=0.0, c=None, row_server=None,
                       pack=None, want_grad=True, want_proj=True, **weights):
    """One evaluation of N rows in one launch (mp_kp_objective).  params (N, 85), targets (N, K, 2), conf (N, K) confidences (or
    c (N, K) ready weights), prev (N, 75) = [transl, thetas] of the temporal target or None (no temporal term).  servers: one
    SMPLServer, or a list with row_server (N,) naming each row's (default: row n uses servers[n]).  Returns a dict: terms (N, 3) =
    [L2d, Lt, w_2d L2d + w_t Lt], grad (N, 85) of the total, proj (N, K, 2), flags (N,) int32 (1: a keypoint had z_c <= 0; it
    contributed nothing and projects to 0).  No host synchronisation."""
    if c is None:
        c = keypoint_weights(conf, kmap, conf_threshold)
    pack, params, targets, c, prev, cam, rt, N = _inputs(servers, params, targets, c, kmap, camera, prev, row_server, pack)
    f32 = dict(dtype=torch.float32, device=pack.device)
    out = {"terms": torch.empty(N, 3, **f32), "flags": torch.zeros(N, dtype=torch.int32, device=pack.device),
           "grad": torch.empty(N, N_PARAMS, **f32) if want_grad else None,
           "proj": torch.empty(N, kmap.K, 2, **f32) if want_proj else None}
    rho, w_2d, w_t, w_p = _weights(weights)
    k = pack
    hip.lib().mp_kp_objective(k.parents, k.j_template, k.j_shapedirs, k.sv_template, k.s_shapedirs, k.s_posedirs, k.s_weights,
                              k.n_tables, rt, k.map_ptr, k.map_idx, k.map_w, k.tmap_ptr, k.tmap_k, k.tmap_w, kmap.S, kmap.K, params,
                              prev, targets, c, cam, N, rho, w_2d, w_t, w_p, out["terms"], out["grad"], out["proj"], out["flags"],
                              hip.stream())
    return out


def project_keypoints(servers, params, kmap, camera, row_server=None, pack=None):
    """the keypoints (N, K, 2) of params (N, 85) under camera, and flags (N,)"""
    params = torch.as_tensor(params)
    if params.dim() != 2:
        raise ValueError(f"params: expected (N, {N_PARAMS}), got {tuple(params.shape)}")
    N = params.shape[0]
    z = torch.zeros(N, kmap.K, 2)
    out = keypoint_objective(servers, params, z, None, kmap, camera, c=z[..., 0], row_server=row_server, pack=pack, want_grad=False)
    return out["proj"], out["flags"]


def refine_frame(servers, start, targets, c, camera, kmap, prev=None, iters=150, lr=1e-3, history=False, row_server=None, pack=None,
                 beta1=ADAM["beta1"], beta2=ADAM["beta2"], eps=ADAM["eps"], **weights):
    """iters Adam steps on the rows of one frame in ONE launch (mp_kp_fit).  start (P, 85), targets (P, K, 2), c (P, K) from
    keypoint_weights, prev (P, 75) or None.  lr: one value or (lr_transl, lr_pose, lr_betas), torch's parameter groups.  Returns a
    dict: params (P, 85), flags (P,), history (P, iters, 3) = the terms before each step (None unless asked for)."""
    pack, start, targets, c, prev, cam, rt, N = _inputs(servers, start, targets, c, kmap, camera, prev, row_server, pack)
    iters = int(iters)
    if iters < 0:
        raise ValueError(f"iters must not be negative, got {iters}")
    lrs = (float(lr),) * 3 if np.ndim(lr) == 0 else tuple(float(x) for x in lr)
    if len(lrs) != 3:
        raise ValueError(f"lr: expected one value or (transl, pose, betas), got {lr}")
    f32 = dict(dtype=torch.float32, device=pack.device)
    out = {"params": torch.empty(N, N_PARAMS, **f32), "flags": torch.zeros(N, dtype=torch.int32, device=pack.device),
           "history": torch.empty(N, iters, 3, **f32) if history else None}
    rho, w_2d, w_t, w_p = _weights(weights)
    k = pack
    hip.lib().mp_kp_fit(k.parents, k.j_template, k.j_shapedirs, k.sv_template, k.s_shapedirs, k.s_posedirs, k.s_weights, k.n_tables,
                        rt, k.map_ptr, k.map_idx, k.map_w, k.tmap_ptr, k.tmap_k, k.tmap_w, kmap.S, kmap.K, start, prev, targets, c,
                        cam, N, rho, w_2d, w_t, w_p, iters, lrs[0], lrs[1], lrs[2], beta1, beta2, eps, out["params"], out["history"],
                        out["flags"], hip.stream())
    return out


# ------------------------------------------------------------------------------------------------ the reference's frame loop
def sequence_loop(init, tracked, interpolate_frames, fit):
    """The sequencing of preprocessing_multiple_trace.py:360-527 around `fit`, device-agnostic torch.  init (F, P, 85); tracked
    (F, P) bool; fit(f, start (P, 85), prev (P, 75)) -> (P, 85).  Frame f starts from its initial values, or from frame f - 1's
    result for tracked pairs (f >= 1); its temporal target is frame f - 1's result (frame 0: its own start); an interpolated frame
    copies the target's pose and translation and keeps its start betas without optimising.  Returns results (F, P, 85) and the
    temporal targets (F, P, 75)."""
    F = init.shape[0]
    interp = {int(f) for f in interpolate_frames}
    results, prevs = [], []
    for f in range(F):
        start = init[f]
        if f > 0:
            start = torch.where(tracked[f][:, None], results[-1], start)
        prev = (results[-1] if f > 0 else start)[:, :75]
        prevs.append(prev)
        results.append(torch.cat([prev, start[:, 75:]], 1) if f in interp else fit(f, start, prev))
    return torch.stack(results), torch.stack(prevs)


def _seq_inputs(init, keypoints, kmap, conf_threshold, tracking, interpolate_frames, second_set):
    try:
        pose, trans, shape = (torch.as_tensor(init[k]).detach() for k in ("pose", "trans", "shape"))
    except (KeyError, TypeError, IndexError):
        raise ValueError("init: expected a dict with 'pose' (F, P, 72), 'trans' (F, P, 3), 'shape' (F, P, 10)") from None
    if pose.dim() != 3 or pose.shape[2] != 72 or min(pose.shape[:2]) < 1:
        raise ValueError(f"init['pose']: expected (F, P, 72), got {tuple(pose.shape)}")
    F, P = pose.shape[:2]
    if tuple(trans.shape) != (F, P, 3) or tuple(shape.shape) != (F, P, 10):
        raise ValueError(f"init: expected trans ({F}, {P}, 3) and shape ({F}, {P}, 10), got {tuple(trans.shape)} and {tuple(shape.shape)}")
    for k, a in (("pose", pose), ("trans", trans), ("shape", shape)):
        if not a.dtype.is_floating_point:
            raise ValueError(f"init[{k!r}]: expected floating point, got {a.dtype} with shape {tuple(a.shape)}")
    sets = [(keypoints, kmap.K)]
    if second_set is not None:
        sets.append((second_set["keypoints"], second_set["kmap"].K))
        kmap = kmap.concat(second_set["kmap"])
        conf_threshold = (float(conf_threshold), float(second_set.get("conf_threshold", 0.4)))
    kps = []
    for i, (kp, Ks) in enumerate(sets):
        kp = torch.as_tensor(kp).detach()
        if tuple(kp.shape) != (F, P, Ks, 3) or not kp.dtype.is_floating_point:
            raise ValueError(f"keypoints{' (second set)' if i else ''}: expected floating-point ({F}, {P}, {Ks}, 3) = (u, v, "
                             f"confidence), got {tuple(kp.shape)} {kp.dtype}")
        kps.append(kp.float())
    kp = torch.cat(kps, 2)
    tracked = torch.zeros(F, P, dtype=torch.bool)
    for pair in tracking:
        f, p = (int(x) for x in pair)
        if not (0 <= f < F and 0 <= p < P):
            raise ValueError(f"tracking: (frame, person) = ({f}, {p}) outside ({F}, {P})")
        tracked[f, p] = True
    for f in interpolate_frames:
        if not 0 <= int(f) < F:
            raise ValueError(f"interpolate_frames: frame {f} outside [0, {F})")
    init85 = pack_params(pose.float(), trans.float(), shape.float())
    return init85, kp[..., :2].contiguous(), keypoint_weights(kp[..., 2], kmap, conf_threshold), tracked, kmap, F, P


def refine_sequence(servers, init, keypoints, camera, kmap, iters=150, lr=1e-3, conf_threshold=0.6, interpolate_frames=(),
                    tracking=(), second_set=None, pack=None, **weights):
    """The reference's refine loop over a sequence.  servers: one SMPLServer per person; init: dict of pose (F, P, 72), trans
    (F, P, 3), shape (F, P, 10) (the per-frame initial values); keypoints (F, P, K, 3) = (u, v, confidence) in kmap's order;
    tracking: (frame, person) pairs that start from the previous frame's result; interpolate_frames: frames that copy it;
    second_set: dict(keypoints (F, P, K2, 3), kmap, conf_threshold=0.4), a second detector's keypoints with their own K_set.
    Everything is uploaded once, every frame is one launch on the current stream, and nothing synchronises until the caller reads
    the results: a dict of pose (F, P, 72), trans (F, P, 3), shape (F, P, 10), terms (F, P, 3) = [L2d, Lt, total] at the refined
    parameters against each frame's temporal target, flags (F, P)."""
    init85, targets, c, tracked, kmap_all, F, P = _seq_inputs(init, keypoints, kmap, conf_threshold, tracking, interpolate_frames,
                                                              second_set)
    servers = list(servers) if isinstance(servers, (list, tuple)) else [servers]
    if len(servers) not in (1, P):
        raise ValueError(f"servers: expected one per person ({P}) or one for all, got {len(servers)}")
    if second_set is not None or pack is None:
        pack = kmap_all.pack(servers)
    dev = pack.device
    init85, targets, c, tracked = init85.to(dev), targets.to(dev), c.to(dev), tracked.to(dev)
    cam = camera_rows(camera, P, dev)
    rs = None if len(servers) == 1 else np.arange(P)
    flags = []

    def fit(f, start, prev):
        out = refine_frame(servers, start, targets[f], c[f], cam, kmap_all, prev, iters, lr, row_server=rs, pack=pack, **weights)
        flags.append((f, out["flags"]))
        return out["params"]

    res, prevs = sequence_loop(init85, tracked, interpolate_frames, fit)
    fin = keypoint_objective(servers, res.reshape(F * P, N_PARAMS), targets.reshape(F * P, -1, 2), None, kmap_all,
                             cam.repeat(F, 1), prevs.reshape(F * P, 75), c=c.reshape(F * P, -1),
                             row_server=None if rs is None else np.tile(rs, F), pack=pack, want_grad=False, want_proj=False, **weights)
    fl = fin["flags"].reshape(F, P).clone()
    for f, x in flags:
        fl[f] |= x
    pose, trans, shape = split_params(res)
    return {"pose": pose.contiguous(), "trans": trans.contiguous(), "shape": shape.contiguous(), "terms": fin["terms"].reshape(F, P, 3),
            "flags": fl, "prev": prevs}
