"""SMPL body model on the device: table loading and the SMPLServer module API.

Mirrors the constructor / attribute / forward contract of the reference's SMPLServer (code/lib/model/smpl.py:6-94) and
of the SMPL class it wraps (code/lib/smpl/body_models.py:60-365) for what the hot path and its callers read:
`verts_c`, `joints_c`, `tfs_c_inv`, `faces`, `smpl.faces`, `bone_parents`, `param_canonical`, and
forward(scale, transl, thetas, betas, absolute=False) -> {'smpl_verts','smpl_tfs','smpl_jnts','smpl_all_jnts',
'smpl_weights'}; the SMPL sub-module's parameters / buffers keep the reference's state-dict names.
The arithmetic (blend shapes, Rodrigues, kinematic chain, LBS) and its adjoint (mp_smpl_pose, mp_smpl_verts_bwd,
mp_smpl_pose_bwd_lbs) run in csrc/smpl.hip.  Beyond the reference: pose_batch(params (N, 86)) poses N rows in two launches
(mp_smpl_pose_batch, forward only) for callers that need many bodies at once (pose_metrics.pose_sequence).
"""
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

from . import hip

NUM_VERTS, NUM_JOINTS = 6890, 24


def _to_np(a, dtype=np.float32):
    if "scipy.sparse" in str(type(a)):
        a = a.todense()
    if hasattr(a, "r"):  # chumpy arrays of the licensed pickle
        a = a.r
    return np.array(a, dtype=dtype)


def load_smpl_tables(gender="neutral", model_dir=None):
    """Reads SMPL_{GENDER}.pkl from `model_dir`, $MULTIPLY_SMPL_DIR or ./lib/smpl/smpl_model (the reference's location,
    smpl.py:13); falls back to the seeded synthetic tables only when MULTIPLY_SYNTHETIC_SMPL=1 is set explicitly."""
    dirs = [model_dir, os.environ.get("MULTIPLY_SMPL_DIR"), os.path.join(os.getcwd(), "lib/smpl/smpl_model")]
    for d in dirs:
        if d and os.path.exists(os.path.join(d, f"SMPL_{str(gender).upper()}.pkl")):
            with open(os.path.join(d, f"SMPL_{str(gender).upper()}.pkl"), "rb") as f:
                return pickle.load(f, encoding="latin1")
    if os.environ.get("MULTIPLY_SYNTHETIC_SMPL") == "1":
        from .synthetic import make_smpl_tables
        return make_smpl_tables(0)
    raise FileNotFoundError("SMPL model file not found (set MULTIPLY_SMPL_DIR, or MULTIPLY_SYNTHETIC_SMPL=1 for the "
                            "synthetic body used by the benchmarks)")


class SMPLDeviceTables:
    """fp32 device copies of the model tables in the layouts the kernels read."""

    def __init__(self, tables, device):
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.v_template = f(_to_np(tables["v_template"]))                                   # (V,3)
        self.shapedirs = f(_to_np(np.asarray(tables["shapedirs"])[:, :, :10]))               # (V,3,10)
        pd = _to_np(tables["posedirs"])
        self.posedirs = f(np.ascontiguousarray(pd.reshape(-1, pd.shape[-1]).T))              # (207, 3V)
        self.j_regressor = f(_to_np(tables["J_regressor"]))                                  # (24,V)
        self.lbs_weights = f(_to_np(tables["weights"]))                                      # (V,24)
        parents = _to_np(tables["kintree_table"], np.float64)[0].astype(np.int64)
        parents[0] = -1
        self.parents_np = parents
        self.parents = f(parents.astype(np.int32))
        self.faces = np.asarray(tables["f"]).astype(np.int64)
        # d rest-joints / d betas (J = J_regressor (v_template + shapedirs betas)): a constant table, used by the
        # pose/shape backward (mp_smpl_pose_bwd)
        self.j_shapedirs = torch.einsum("jv,vkl->jkl", self.j_regressor, self.shapedirs).contiguous()   # (24,3,10)
        assert self.v_template.shape == (NUM_VERTS, 3) and self.lbs_weights.shape == (NUM_VERTS, NUM_JOINTS)


def knn_cluster_perm(verts_np):
    """Static clustering for the exact nearest-vertex search: vertices are split kd-tree style into leaves of exactly 2 KNN_CLUSTER
    (the last one partial) so that clusters stay spatially compact under posing, and every leaf once more into two halves of at most
    KNN_CLUSTER (32): the fine clusters the eval searches scan; the leaves themselves -- the pairs (2c, 2c + 1) -- are the coarse
    clusters of the training searches (csrc/geom.hip k_knn_build).  Returns int32 [KNN_NC * KNN_CLUSTER], -1 = padding."""
    CL = hip.KNN_CLUSTER
    leaves = []

    def split(idx):
        pts = verts_np[idx]
        axis = int(np.argmax(pts.max(0) - pts.min(0)))
        order = idx[np.argsort(pts[:, axis], kind="stable")]
        if len(idx) <= 2 * CL:
            leaves.append(order[:CL])
            leaves.append(order[CL:])
            return
        nleaf = -(-len(idx) // (2 * CL))
        nl = (nleaf // 2) * 2 * CL
        split(order[:nl])
        split(order[nl:])

    split(np.arange(verts_np.shape[0]))
    assert len(leaves) <= hip.KNN_NC and hip.KNN_NC % 2 == 0
    perm = -np.ones(hip.KNN_NC * CL, dtype=np.int32)
    for c, l in enumerate(leaves):
        perm[c * CL:c * CL + len(l)] = l
    return perm


FACE_KEYPOINT_VERTS = (332, 6260, 2800, 4071, 583)   # nose, reye, leye, rear, lear (lib/smpl/vertex_ids.py 'smplh')


class _VertexJointSelector(nn.Module):
    """lib/smpl/vertex_joint_selector.py with use_hands=False, use_feet_keypoints=False (smpl.py:12-17): the five face
    keypoints appended to the 24 kinematic joints."""

    def __init__(self, device):
        super().__init__()
        self.register_buffer("extra_joints_idxs", torch.tensor(FACE_KEYPOINT_VERTS, dtype=torch.long, device=device))


class _SMPLModule(nn.Module):
    """Stands in for `smpl_server.smpl` (lib/smpl/body_models.py SMPL): callers read `.faces` / `.bone_parents`, and its
    registered parameters / buffers are part of the checkpoint contract -- the reference's state dict carries
    `smpl_server_list.N.smpl.{betas,global_orient,body_pose,transl,faces_tensor,v_template,shapedirs,J_regressor,posedirs,
    parents,lbs_weights}` and `...smpl.vertex_joint_selector.extra_joints_idxs` (body_models.py:152-249), the same again
    under `deformer_list.N.smpl.smpl.`.  The buffers ALIAS the device tables the kernels read (same shapes and layouts as
    the reference's), so a loaded checkpoint's tables are the ones used."""

    def __init__(self, tables):
        super().__init__()
        dev = tables.v_template.device
        self.faces = tables.faces
        self.bone_parents = tables.parents_np.copy()
        self.vertex_joint_selector = _VertexJointSelector(dev)
        self.register_buffer("faces_tensor", torch.from_numpy(tables.faces).to(dev))
        z = lambda n: nn.Parameter(torch.zeros(1, n, dtype=torch.float32, device=dev), requires_grad=True)
        self.betas, self.global_orient, self.body_pose, self.transl = z(10), z(3), z(69), z(3)   # body_models.py:158-211
        self.register_buffer("v_template", tables.v_template)
        self.register_buffer("shapedirs", tables.shapedirs)
        self.register_buffer("J_regressor", tables.j_regressor)
        self.register_buffer("posedirs", tables.posedirs)
        self.register_buffer("parents", torch.from_numpy(tables.parents_np.copy()).to(dev))          # long, parents[0] = -1
        self.register_buffer("lbs_weights", tables.lbs_weights)
        self._register_load_state_dict_pre_hook(self._check_tables)

    _TABLE_KEYS = ("v_template", "shapedirs", "J_regressor", "posedirs", "lbs_weights", "parents", "faces_tensor")

    def _check_tables(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Everything derived from the tables at construction (canonical vertices and inverse bone transforms, the joint
        shape basis, the nearest-vertex cluster order, the canonical meshes) is NOT rebuilt by load_state_dict: a
        checkpoint whose body-model tables differ from the ones this model was built with (another gender, synthetic
        tables) is refused here instead of leaving the model silently inconsistent."""
        for k in self._TABLE_KEYS:
            v = state_dict.get(prefix + k)
            if v is None:
                continue
            cur = getattr(self, k)
            same = tuple(v.shape) == tuple(cur.shape) and bool(
                torch.equal(v.to(cur.device).to(cur.dtype), cur) if not cur.is_floating_point()
                else torch.allclose(v.to(cur.device).to(cur.dtype), cur, rtol=0, atol=1e-7))
            if not same:
                error_msgs.append(f"{prefix}{k}: the checkpoint's SMPL table differs from the one this model was constructed with "
                                  f"(gender / betas_path / smpl_tables); construct the model with the checkpoint's body model")


class _PoseLBS(torch.autograd.Function):
    """smpl_verts (V,3), smpl_jnts (24,3), smpl_all_jnts (29,3) and smpl_tfs (24,4,4) of the 86 parameters: ONE node over the
    forward launches of mp_smpl_pose, whose backward takes any subset of the four upstream gradients (SMPLServer.pose_backward:
    csrc/smpl.hip mp_smpl_verts_bwd, mp_smpl_pose_bwd_lbs).  smpl_all_jnts = the joints + the face-keypoint
    vertices, so its gradient folds into d joints and d verts."""

    @staticmethod
    def forward(ctx, server, p):
        prm = p.detach().contiguous()
        dev = prm.device
        verts = torch.empty(NUM_VERTS, 3, dtype=torch.float32, device=dev)
        jnts = torch.empty(NUM_JOINTS, 3, dtype=torch.float32, device=dev)
        tfs = torch.empty(NUM_JOINTS, 4, 4, dtype=torch.float32, device=dev)
        server.pose_into(prm, verts, tfs, jnts)
        all_jnts = torch.cat([jnts, verts[server.smpl.vertex_joint_selector.extra_joints_idxs]], 0)
        # v_shaped / J / A / pose feature of THIS call (the server's work buffer is reused by the next pose_into)
        ctx.server, ctx.prm, ctx.work = server, prm, server._work.clone()
        ctx.set_materialize_grads(False)
        return verts, jnts, all_jnts, tfs

    @staticmethod
    def backward(ctx, dverts, djnts, dall, dtfs):
        return None, ctx.server.pose_backward(ctx.prm, ctx.work, dverts=dverts, djoints=djnts, dall_joints=dall, dtfs=dtfs)


class SMPLServer(nn.Module):
    def __init__(self, gender="neutral", betas=None, v_template=None, smpl_tables=None, device=None):
        super().__init__()
        if v_template is not None:
            raise NotImplementedError("custom v_template is not used by the shipped configs")
        hip.require_device()
        device = torch.device(device or "cuda")
        raw = smpl_tables if smpl_tables is not None else load_smpl_tables(gender)
        self.tables = raw if isinstance(raw, SMPLDeviceTables) else SMPLDeviceTables(raw, device)
        self.smpl = _SMPLModule(self.tables)
        self.faces = self.tables.faces
        self.bone_parents = self.tables.parents_np.astype(int)
        self.bone_ids = [[int(self.bone_parents[i]), i] for i in range(NUM_JOINTS)]
        self.v_template = None
        self.betas = None if betas is None else torch.tensor(np.asarray(betas), dtype=torch.float32, device=device)
        pc = torch.zeros(1, 86, dtype=torch.float32, device=device)
        pc[0, 0] = 1
        pc[0, 9] = np.pi / 6
        pc[0, 12] = -np.pi / 6
        if self.betas is not None:
            pc[0, -10:] = self.betas
        self.param_canonical = pc
        self._work = torch.empty(3 * NUM_VERTS + 1024, dtype=torch.float32, device=device)
        self.tfs_c_inv = None
        out = self.forward(*torch.split(pc, [1, 3, 72, 10], dim=1), absolute=True)
        self.verts_c = out["smpl_verts"]
        self.joints_c = out["smpl_jnts"]
        self.tfs_c_inv = torch.linalg.inv(out["smpl_tfs"].squeeze(0)).contiguous()   # init-time only (smpl.py:47)

    def pose_into(self, params86, verts, tfs, joints, absolute=False, work=None):
        """raw launch: params86 (86,) device -> preallocated verts (V,3), tfs (24,4,4), joints (24,3); `work` (3V + 1024
        floats) defaults to the server's own buffer"""
        t = self.tables
        hip.lib().mp_smpl_pose(t.v_template, t.shapedirs, t.posedirs, t.j_regressor, t.lbs_weights, t.parents, params86,
                               None if absolute else self.tfs_c_inv, verts, tfs, joints, self._work if work is None else work,
                               hip.stream())

    POSE_BATCH_OUTPUTS = ("verts", "joints", "tfs")

    def pose_batch(self, params, absolute=False, want=POSE_BATCH_OUTPUTS, rows_per_call=None):
        """N parameter rows at once (mp_smpl_pose_batch: two launches whatever N is, posedirs read once per call instead of once
        per row).  params (N, 86) = [scale, transl 3, thetas 72, betas 10] per row -> a dict with the entries named in `want`:
        verts (N, V, 3), joints (N, 24, 3), tfs (N, 24, 4, 4); the values per row are forward()'s (absolute as there), and a row
        has the same bits alone and inside any batch.  rows_per_call bounds the rows of one kernel call (its work buffer is
        hip.SMPL_BATCH_ROW_WORK floats per row; the outputs are allocated whole).  FORWARD ONLY: it runs under no_grad on
        detached inputs and nothing it returns carries a gradient -- optimise poses through forward()."""
        want = tuple(want)
        bad = [w for w in want if w not in self.POSE_BATCH_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want: a non-empty subset of {self.POSE_BATCH_OUTPUTS}, got {want}")
        if not torch.is_tensor(params) or params.dim() != 2 or params.shape[1] != 86:
            raise ValueError(f"params: expected a (N, 86) tensor, got {tuple(params.shape) if torch.is_tensor(params) else type(params)}")
        if rows_per_call is not None and int(rows_per_call) < 1:
            raise ValueError(f"rows_per_call must be at least 1, got {rows_per_call}")
        with torch.no_grad():
            t, dev = self.tables, self.param_canonical.device
            prm = params.detach().to(device=dev, dtype=torch.float32).contiguous()
            N = prm.shape[0]
            f32 = dict(dtype=torch.float32, device=dev)
            out = {}
            if "verts" in want:
                out["verts"] = torch.empty(N, NUM_VERTS, 3, **f32)
            if "joints" in want:
                out["joints"] = torch.empty(N, NUM_JOINTS, 3, **f32)
            if "tfs" in want:
                out["tfs"] = torch.empty(N, NUM_JOINTS, 4, 4, **f32)
            step = N if rows_per_call is None else int(rows_per_call)
            work = torch.empty(max(min(step, N), 1) * hip.SMPL_BATCH_ROW_WORK, **f32)
            for s in range(0, N, max(step, 1)):
                e = min(N, s + step)
                part = lambda k: out[k][s:e] if k in out else None
                hip.lib().mp_smpl_pose_batch(t.v_template, t.shapedirs, t.posedirs, t.j_regressor, t.lbs_weights, t.parents,
                                             prm[s:e], e - s, None if absolute else self.tfs_c_inv, part("verts"), part("tfs"),
                                             part("joints"), work, hip.stream())
        return out

    def pose_backward(self, params86, work=None, dverts=None, djoints=None, dall_joints=None, dtfs=None):
        """Adjoint of forward(absolute=False) -> d params (86,) = [scale, transl 3, thetas 72, betas 10].  Upstreams (any may
        be None): dverts (V,3), djoints (24,3), dall_joints (29,3), dtfs (24,4,4).  `work`: the work buffer of the pose_into
        call that produced the outputs; None = pose again into a private buffer (same launches, same values).  Deterministic:
        the same inputs give bit-identical gradients."""
        t, dev = self.tables, params86.device
        f32 = dict(dtype=torch.float32, device=dev)
        prm = params86.detach().float().contiguous()
        if work is None:
            work = torch.empty_like(self._work)
            self.pose_into(prm, torch.empty(NUM_VERTS, 3, **f32), torch.empty(NUM_JOINTS, 4, 4, **f32),
                           torch.empty(NUM_JOINTS, 3, **f32), work=work)
        flat = lambda g, n: None if g is None else g.detach().reshape(n, -1).float().contiguous()
        dverts, djoints, dall_joints, dtfs = flat(dverts, NUM_VERTS), flat(djoints, NUM_JOINTS), flat(dall_joints, NUM_JOINTS + len(FACE_KEYPOINT_VERTS)), flat(dtfs, NUM_JOINTS)
        if dall_joints is not None:         # smpl_all_jnts = [joints; verts[face keypoints]] (five distinct vertices)
            djoints = dall_joints[:NUM_JOINTS] if djoints is None else djoints + dall_joints[:NUM_JOINTS]
            dverts = torch.zeros(NUM_VERTS, 3, **f32) if dverts is None else dverts.clone()
            dverts[self.smpl.vertex_joint_selector.extra_joints_idxs] += dall_joints[NUM_JOINTS:]
        dA = dpf = din = None
        if dverts is not None:
            dlbs = torch.empty(hip.SMPL_DLBS, **f32)
            scratch = torch.empty(hip.SMPL_VBWD_SCRATCH, **f32)
            hip.lib().mp_smpl_verts_bwd(t.posedirs, t.shapedirs, t.lbs_weights, prm, work, dverts, scratch, dlbs, hip.stream())
            dA, dpf, din = dlbs[:NUM_JOINTS * 16], dlbs[NUM_JOINTS * 16:NUM_JOINTS * 16 + 207], dlbs[NUM_JOINTS * 16 + 207:]
        dprm = torch.empty(86, **f32)
        rest = work[3 * NUM_VERTS:3 * NUM_VERTS + 3 * NUM_JOINTS]          # csrc/smpl.hip W_J
        hip.lib().mp_smpl_pose_bwd_lbs(t.parents, prm, self.tfs_c_inv, rest, t.j_shapedirs, dtfs, dA, djoints, dpf, din, dprm,
                                       hip.stream())
        return dprm

    def rest_joints(self):
        """J (24,3) of the most recent pose_into() call (kernel work buffer, csrc/smpl.hip W_J)"""
        return self._work[3 * NUM_VERTS:3 * NUM_VERTS + 3 * NUM_JOINTS].clone()

    def forward(self, scale, transl, thetas, betas, absolute=False):
        """smpl.py:50-94.  When any of scale / transl / thetas / betas requires grad (and absolute=False), smpl_verts,
        smpl_jnts, smpl_all_jnts and smpl_tfs all carry gradients to them, as in the reference (the mesh-space losses and
        keypoint terms back-propagate into BodyModelParams, multiply_model.py:586-620, 969-974): one autograd node
        (_PoseLBS) over the same forward launches, so the values are those of the no-grad call."""
        dev = self.param_canonical.device
        p = torch.cat([scale.reshape(1, 1), transl.reshape(1, 3), thetas.reshape(1, 72), betas.reshape(1, 10)], 1)
        p = p.float().reshape(86)
        if torch.is_grad_enabled() and p.requires_grad and not absolute:
            verts, jnts, all_jnts, tfs = _PoseLBS.apply(self, p)
        else:
            verts = torch.empty(NUM_VERTS, 3, dtype=torch.float32, device=dev)
            jnts = torch.empty(NUM_JOINTS, 3, dtype=torch.float32, device=dev)
            tfs = torch.empty(NUM_JOINTS, 4, 4, dtype=torch.float32, device=dev)
            self.pose_into(p.detach().contiguous(), verts, tfs, jnts, absolute=absolute)
            # smpl_all_jnts: the 24 kinematic joints + the face keypoint vertices (body_models.py:345; smpl.py:83-84) -- the
            # vertices are already scaled / translated exactly like the joints (smpl.py:77-84)
            all_jnts = torch.cat([jnts, verts[self.smpl.vertex_joint_selector.extra_joints_idxs]], 0)
        return {"smpl_verts": verts[None], "smpl_jnts": jnts[None], "smpl_all_jnts": all_jnts[None], "smpl_tfs": tfs[None],
                "smpl_weights": self.tables.lbs_weights[None]}
