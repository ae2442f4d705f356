"""Pose metrics over a sequence: how close estimated bodies are to ground-truth bodies.

The method this project restates is judged, for pose, on four numbers over a whole sequence against ground-truth SMPL bodies.  The
reference ships no code for them, so the definitions are the published ones, spelled out.  An ITEM is one person of one frame: n
predicted points p_i (joints or vertices) and the n ground-truth points x_i they correspond to.

  mpjpe_global  mean |p_i - x_i| over the joints of an item.
  mpjpe         the same after moving both sets to their own root joint: mean |(p_i - p_root) - (x_i - x_root)|, root = joint
                `root` (0, the pelvis).  This is what is usually reported as MPJPE.
  pa_mpjpe      mean |s R p_i + t - x_i| where (s, R, t) minimises the summed squares over similarity transforms with
                det R = +1 (Umeyama 1991): H = sum (p_i - mean p)(x_i - mean x)^T = U S V^T, D = diag(1, 1, sign det(V U^T)),
                R = V D U^T, s = tr(S D) / sum |p_i - mean p|^2, t = mean x - s R mean p.  A mirrored body is NOT aligned.
  mve_global, mve, pa_mve
                the same three over the vertices; mve is aligned by the JOINTS' root (the pelvis-aligned convention), not by a vertex.
  cd            contact distance: a correspondence (frame, person a, vertex of a, person b, face of b, barycentrics) marks a point of
                a's surface that touches b's in the ground truth; its distance on a set of bodies is
                |v[f, a, vertex] - sum_k bary_k v[f, b, faces[face, k]]|.  cd is the mean over all correspondences on the PREDICTED
                bodies, cd_gt the same on the ground truth (near 0 by construction); both also per frame (NaN where a frame has
                none).  contacts_from_bodies builds correspondences from ground-truth bodies.
  pcdr          percentage of correct depth relations.  z[f, p] is the depth of person p's root joint: the third camera coordinate
                under `view` ((3, 4) or (F, 3, 4), world to camera), the world z without one.  For every frame and unordered pair
                p < q, d = z_p - z_q and rel(d) = 0 where unit_scale |d| < depth_threshold, else sign(d); pcdr is the share of
                pairs whose predicted relation equals the ground truth's.  One person: NaN, count 0.
  left out      an item with a non-finite coordinate has NaN in all its values; an item whose predicted points all coincide has
                NaN in its Procrustes value (there is no scale).  Both are counted, none fails the call.
  sequence      the mean of the per-item values over the items where the value is defined (not NaN).

Prediction and ground truth must ALREADY SHARE A FRAME OF REFERENCE (camera or world: nothing here aligns the two), and persons are
PAIRED BY INDEX: person p of the prediction is scored against person p of the ground truth.  Only the *_global metrics, cd and pcdr
depend on the frame of reference; the root- and Procrustes-aligned ones do not.  The joints are the 24 kinematic joints of the body
model unless a `joint_regressor` is given: PUBLISHED NUMBERS MAY USE ANOTHER JOINT SET (the 14 LSP or 17 H36M joints regressed from
the vertices), and are comparable only when the same regressor is passed here.

The per-item means and the contact distances are device kernels (csrc/pose_metrics.hip: sums and the 3 x 3 SVD in double on the
float32 inputs, fixed order); the bodies come from SMPLServer.pose_batch (csrc/smpl.hip mp_smpl_pose_batch); the depth relations are
P (P - 1) / 2 comparisons per frame in torch.  Nothing here is differentiable.  This module imports without a device."""
import math

import numpy as np
import torch

from . import hip

DISTANCE_KEYS = ("mpjpe", "mpjpe_global", "pa_mpjpe", "mve", "mve_global", "pa_mve")


def params_from_body_models(body_model_list, scale=1.0):
    """(F, P, 86) float32 = [scale, transl 3, global_orient 3 + body_pose 69, betas 10] from one BodyModelParams per person (the
    rows of every frame; the person's single betas row repeated), detached, on the tables' device"""
    rows = []
    for bm in body_model_list:
        go, bp, tr, be = (getattr(bm, k).weight.detach().float() for k in ("global_orient", "body_pose", "transl", "betas"))
        F = go.shape[0]
        rows.append(torch.cat([torch.full((F, 1), float(scale), dtype=torch.float32, device=go.device), tr, go, bp,
                               be[:1].expand(F, 10)], 1))
    if not rows:
        raise ValueError("body_model_list: expected at least one BodyModelParams")
    if len({r.shape[0] for r in rows}) != 1:
        raise ValueError(f"body_model_list: the persons differ in their number of frames: {[r.shape[0] for r in rows]}")
    return torch.stack(rows, 1).contiguous()


def _tensor(x):
    return x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))


def _check_params(p, name):
    p = _tensor(p).detach()
    if p.dim() != 3 or p.shape[2] != 86 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"{name}: expected parameters (F, P, 86), got {tuple(p.shape)}")
    if not p.dtype.is_floating_point:
        raise TypeError(f"{name}: expected floating-point parameters, got {p.dtype}")
    return p.float()


def _check_servers(servers, P, name):
    if servers is None:
        raise ValueError(f"servers: {name} is given as parameters (F, P, 86), which needs one SMPLServer per person")
    servers = list(servers)
    if len(servers) != P:
        raise ValueError(f"servers: expected one per person ({P}), got {len(servers)}")
    return servers


def pose_sequence(servers, params):
    """Bodies of a whole sequence: params (F, P, 86) -> verts (F, P, V, 3), joints (F, P, 24, 3) float32 on the device.  ONE
    pose_batch call per person, with that person's own tables (servers[p]); forward only."""
    params = _check_params(params, "params")
    F, P = params.shape[0], params.shape[1]
    servers = _check_servers(servers, P, "params")
    verts, joints = [], []
    for p, sv in enumerate(servers):
        out = sv.pose_batch(params[:, p], want=("verts", "joints"))
        verts.append(out["verts"])
        joints.append(out["joints"])
    return torch.stack(verts, 1), torch.stack(joints, 1)


def _check_points(x, name):
    """a prediction / ground truth -> ('params', tensor) or ('points', {joints, verts}) with shapes and dtypes checked"""
    if isinstance(x, dict):
        out = {}
        for k in ("joints", "verts"):
            if x.get(k) is None:
                continue
            t = _tensor(x[k]).detach()
            if t.dim() != 4 or t.shape[3] != 3 or min(t.shape[:3]) < 1:
                raise ValueError(f"{name}[{k!r}]: expected (F, P, n, 3), got {tuple(t.shape)}")
            if t.dtype != torch.float32:
                raise TypeError(f"{name}[{k!r}]: expected float32, got {t.dtype}")
            out[k] = t
        if not out:
            raise ValueError(f"{name}: a dict needs 'joints' (F, P, J, 3) and / or 'verts' (F, P, V, 3)")
        if len(out) == 2 and out["joints"].shape[:2] != out["verts"].shape[:2]:
            raise ValueError(f"{name}: joints {tuple(out['joints'].shape)} and verts {tuple(out['verts'].shape)} differ in (F, P)")
        return "points", out
    return "params", _check_params(x, name)


def _frames_persons(kind, x):
    return tuple(x.shape[:2]) if kind == "params" else tuple(next(iter(x.values())).shape[:2])


def check_contacts(contacts, F, P, V, n_faces):
    """contacts: a dict of HOST arrays frame, person_a, vertex, person_b, face (m,) integers and bary (m, 3) floats -> the same as
    int64 / float32 numpy arrays, every id checked against (F, P, V, n_faces); ValueError / TypeError names the entry"""
    keys = ("frame", "person_a", "vertex", "person_b", "face")
    if not isinstance(contacts, dict) or any(k not in contacts for k in keys + ("bary",)):
        raise ValueError(f"contacts: expected a dict with {keys + ('bary',)}")
    out, m = {}, None
    for k, hi in zip(keys, (F, P, V, P, n_faces)):
        a = contacts[k].detach().cpu().numpy() if torch.is_tensor(contacts[k]) else np.asarray(contacts[k])
        if a.ndim != 1 or (m is not None and a.shape[0] != m):
            raise ValueError(f"contacts[{k!r}]: expected (m,){'' if m is None else f' with m = {m}'}, got {a.shape}")
        if a.dtype.kind not in "iu":
            raise TypeError(f"contacts[{k!r}]: expected integers, got {a.dtype}")
        m = a.shape[0]
        a = a.astype(np.int64)
        if m and (a.min() < 0 or a.max() >= hi):
            raise ValueError(f"contacts[{k!r}]: ids must lie in [0, {hi}), got [{a.min()}, {a.max()}]")
        out[k] = a
    b = contacts["bary"].detach().cpu().numpy() if torch.is_tensor(contacts["bary"]) else np.asarray(contacts["bary"])
    if b.shape != (m, 3) or b.dtype.kind != "f":
        raise ValueError(f"contacts['bary']: expected floats (m, 3) = {(m, 3)}, got {b.dtype} {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError("contacts['bary']: non-finite barycentrics")
    out["bary"] = b.astype(np.float32)
    return out


def _check_faces(faces, V):
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError(f"faces: expected (Nf, 3), got {f.shape}")
    if f.dtype.kind not in "iu":
        raise TypeError(f"faces: expected integers, got {f.dtype}")
    if f.min() < 0 or f.max() >= V:
        raise ValueError(f"faces: vertex ids must lie in [0, {V}), got [{f.min()}, {f.max()}]")
    return np.ascontiguousarray(f.astype(np.int32))


def closest_barycentrics(p, tri):
    """barycentric coordinates (n, 3) float64 of the point of triangle tri[i] (n, 3, 3) closest to p[i] (n, 3): the Voronoi regions
    of the triangle (Ericson, Real-Time Collision Detection 5.1.5) -- vertex, edge, interior -- in double by torch; clamped at 0 and
    renormalised against the last rounding.  A face of zero area that is a point or a segment still has an answer (the regions
    before the interior catch it)."""
    p, tri = p.double(), tri.double()
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    dot = lambda x, y: (x * y).sum(1)
    ab, ac = b - a, c - a
    d1, d2 = dot(ab, p - a), dot(ac, p - a)
    d3, d4 = dot(ab, p - b), dot(ac, p - b)
    d5, d6 = dot(ab, p - c), dot(ac, p - c)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    one, zero = torch.ones_like(d1), torch.zeros_like(d1)
    safe = lambda num, den: num / torch.where(den != 0, den, one)
    den = va + vb + vc
    v, w = safe(vb, den), safe(vc, den)
    out = torch.stack([1.0 - v - w, v, w], 1)                                            # interior
    pick = lambda cond, x, y, z: torch.where(cond[:, None], torch.stack([x, y, z], 1), out)
    t = safe(d4 - d3, (d4 - d3) + (d5 - d6))
    out = pick((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), zero, 1.0 - t, t)           # edge bc
    t = safe(d2, d2 - d6)
    out = pick((vb <= 0) & (d2 >= 0) & (d6 <= 0), 1.0 - t, zero, t)                     # edge ac
    out = pick((d6 >= 0) & (d5 <= d6), zero, zero, one)                                  # vertex c
    t = safe(d1, d1 - d3)
    out = pick((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1.0 - t, t, zero)                     # edge ab
    out = pick((d3 >= 0) & (d4 <= d3), zero, one, zero)                                  # vertex b
    out = pick((d1 <= 0) & (d2 <= 0), one, zero, zero)                                   # vertex a
    out = out.clamp(min=0.0)
    return out / out.sum(1, keepdim=True)


def contacts_from_bodies(gt_verts, faces, threshold):
    """Correspondences from ground-truth bodies gt_verts (F, P, V, 3) float32 with the shared face list faces (Nf, 3): for every
    frame and ORDERED pair p != q, the vertices of p whose distance to q's surface is at most `threshold`, each with q's closest
    face and the barycentrics of the closest point on it.  The distance and the face come from the exact closest-face query
    (hip.mesh_closest, through a MeshIndex where hip.mesh_index_wanted says so); the barycentrics are those of the closest point on
    THAT face, formed again in double by torch (closest_barycentrics): the query's own fp32 closest point is right in its distance
    to 16 FLT_EPSILON M but, on the sliver faces a body mesh has, was measured 6e-6 off ALONG the face.  Returns
    the dict pose_metrics takes as `contacts`: host arrays frame, person_a, vertex, person_b, face (m,) int32 and bary (m, 3)
    float32, ordered by frame, then p, then q, then vertex."""
    _, pts = _check_points({"verts": gt_verts}, "gt_verts")
    v = pts["verts"]
    F, P, V = v.shape[:3]
    fc = _check_faces(faces, V)
    if not (float(threshold) >= 0.0 and math.isfinite(float(threshold))):
        raise ValueError(f"threshold must be a finite number >= 0, got {threshold}")
    hip.require_device()
    v = v.cuda().contiguous() if not v.is_cuda else v.contiguous()
    ft = torch.from_numpy(fc.astype(np.int64)).to(v.device)
    use_index = hip.mesh_index_wanted(None, fc.shape[0], ft)
    cols = {k: [] for k in ("frame", "person_a", "vertex", "person_b", "face")}
    bary = []
    for f in range(F):
        for q in range(P):
            fv = v[f, q][ft].contiguous()                                     # (Nf, 3, 3)
            index = hip.MeshIndex(fv) if use_index else None
            for p in range(P):
                if p == q:
                    continue
                d2, face, _ = hip.mesh_closest(v[f, p], fv, index=index, want_point=False)
                sel = torch.nonzero((torch.sqrt(d2.double()) <= float(threshold)) & (face >= 0)).reshape(-1)
                if sel.numel() == 0:
                    continue
                fa = face[sel].long()
                bary.append(closest_barycentrics(v[f, p][sel], fv[fa]).float().cpu().numpy())
                n = sel.numel()
                cols["frame"].append(np.full(n, f, np.int32))
                cols["person_a"].append(np.full(n, p, np.int32))
                cols["person_b"].append(np.full(n, q, np.int32))
                cols["vertex"].append(sel.int().cpu().numpy())
                cols["face"].append(fa.int().cpu().numpy())
    out = {k: (np.concatenate(c) if c else np.zeros(0, np.int32)) for k, c in cols.items()}
    out["bary"] = np.concatenate(bary) if bary else np.zeros((0, 3), np.float32)
    order = np.lexsort((out["vertex"], out["person_b"], out["person_a"], out["frame"]))
    return {k: a[order] for k, a in out.items()}


def depth_relations(z, threshold, unit_scale=1.0):
    """rel (F, P (P - 1) / 2) int8 of the depths z (F, P) for the pairs p < q in row-major order: 0 where unit_scale |z_p - z_q| <
    threshold, else sign(z_p - z_q); and whether the pair's depths are both finite"""
    P = z.shape[1]
    i, j = torch.triu_indices(P, P, 1, device=z.device)
    d = z[:, i] - z[:, j]
    rel = torch.where(float(unit_scale) * d.abs() < float(threshold), torch.zeros_like(d), torch.sign(d))
    return rel.to(torch.int8), torch.isfinite(d)


def _mean(values):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else math.nan


def pose_metrics(pred, gt, servers=None, root=0, joint_regressor=None, unit_scale=1.0, contacts=None, faces=None, view=None,
                 depth_threshold=0.15):
    """MPJPE, MVE, contact distance and PCDR of a predicted sequence against the ground truth -- the definitions of the module's
    docstring.  pred and gt MUST SHARE A FRAME OF REFERENCE and their persons are PAIRED BY INDEX; the joints are the body model's 24
    kinematic joints unless `joint_regressor` is given, and published numbers may use another joint set.

    pred, gt    each either parameters (F, P, 86) = [scale, transl 3, thetas 72, betas 10] (tensor or array; needs `servers`, one
                SMPLServer per person) or a dict with 'joints' (F, P, J, 3) and / or 'verts' (F, P, V, 3) float32 (host or device).
                Ground truth that exists only as joints is scored without a body model; what both sides have is scored.
    root        the root joint of the aligned metrics and of pcdr
    joint_regressor  (K, V) float32: the joints become regressor @ verts on both sides (a torch matmul on the device)
    unit_scale  multiplies every distance (100 for metres -> centimetres), as in metrics.mesh_metrics
    contacts    the dict of contacts_from_bodies (host arrays) -> cd, cd_gt, ...; needs verts on the scored side and `faces`
                (Nf, 3) (default: servers[0].faces)
    view        (3, 4) or (F, 3, 4) world-to-camera rows for pcdr's depths; None: the world z
    depth_threshold  in the scaled unit

    Returns a dict: per-item float64 arrays (F, P) for the keys of DISTANCE_KEYS that both sides allow (mve needs joints for its
    root), their means over the defined items as mean_<key>, n_items, n_left_out_joints / n_left_out_verts (items with a non-finite
    coordinate) and n_degenerate_joints / n_degenerate_verts (no Procrustes scale); pcdr, pcdr_per_frame (F,), n_depth_pairs; with
    contacts cd, cd_gt, cd_per_frame, cd_gt_per_frame (F,), n_contacts_per_frame (F,), n_contacts."""
    # ---- every check first: nothing below this block raises for an argument, nothing in it touches the device
    kp, pred = _check_points(pred, "pred")
    kg, gt = _check_points(gt, "gt")
    F, P = _frames_persons(kp, pred)
    if _frames_persons(kg, gt) != (F, P):
        raise ValueError(f"pred has (F, P) = {(F, P)}, gt {_frames_persons(kg, gt)}")
    if kp == "params" or kg == "params":
        servers = _check_servers(servers, P, "pred" if kp == "params" else "gt")
    from .smpl import NUM_JOINTS, NUM_VERTS
    has = lambda kind, x, k: kind == "params" or k in x
    n_of = lambda kind, x, k: (NUM_VERTS if k == "verts" else NUM_JOINTS) if kind == "params" else x[k].shape[2]
    both_verts = has(kp, pred, "verts") and has(kg, gt, "verts")
    if both_verts and n_of(kp, pred, "verts") != n_of(kg, gt, "verts"):
        raise ValueError(f"pred and gt differ in their number of vertices: {n_of(kp, pred, 'verts')} and {n_of(kg, gt, 'verts')}")
    if joint_regressor is not None:
        joint_regressor = _tensor(joint_regressor).detach()
        if not both_verts:
            raise ValueError("joint_regressor: needs vertices on both sides")
        if joint_regressor.dim() != 2 or joint_regressor.shape[1] != n_of(kp, pred, "verts"):
            raise ValueError(f"joint_regressor: expected (K, V) with V = {n_of(kp, pred, 'verts')}, got {tuple(joint_regressor.shape)}")
        if joint_regressor.dtype != torch.float32:
            raise TypeError(f"joint_regressor: expected float32, got {joint_regressor.dtype}")
        n_joints = joint_regressor.shape[0]
        both_joints = True
    else:
        both_joints = has(kp, pred, "joints") and has(kg, gt, "joints")
        n_joints = n_of(kp, pred, "joints") if both_joints else 0
        if both_joints and n_joints != n_of(kg, gt, "joints"):
            raise ValueError(f"pred and gt differ in their number of joints: {n_joints} and {n_of(kg, gt, 'joints')}")
    if not both_joints and not both_verts:
        raise ValueError("pred and gt have neither joints nor vertices in common")
    if both_joints and not (isinstance(root, (int, np.integer)) and 0 <= int(root) < n_joints):
        raise ValueError(f"root: expected a joint id in [0, {n_joints}), got {root!r}")
    if not (float(unit_scale) > 0.0 and math.isfinite(float(unit_scale))):
        raise ValueError(f"unit_scale must be a positive finite number, got {unit_scale}")
    if not (float(depth_threshold) >= 0.0 and math.isfinite(float(depth_threshold))):
        raise ValueError(f"depth_threshold must be a finite number >= 0, got {depth_threshold}")
    if view is not None:
        view = _tensor(view).detach()
        if tuple(view.shape) not in ((3, 4), (F, 3, 4)):
            raise ValueError(f"view: expected (3, 4) or (F, 3, 4) = {(F, 3, 4)}, got {tuple(view.shape)}")
        if not view.dtype.is_floating_point:
            raise TypeError(f"view: expected floating point, got {view.dtype}")
    if contacts is not None:
        if not both_verts:
            raise ValueError("contacts: needs vertices on both sides")
        if faces is None and servers is not None:
            faces = list(servers)[0].faces
        if faces is None:
            raise ValueError("faces: contacts need the bodies' face list (Nf, 3)")
        V = n_of(kp, pred, "verts")
        faces = _check_faces(faces, V)
        contacts = check_contacts(contacts, F, P, V, faces.shape[0])

    # ---- the bodies
    hip.require_device()
    with torch.no_grad():
        def resolve(kind, x):
            if kind == "params":
                v, j = pose_sequence(servers, x)
                return {"verts": v, "joints": j}
            return dict(x)
        pred, gt = resolve(kp, pred), resolve(kg, gt)
        dev = next((t.device for d in (pred, gt) for t in d.values() if t.is_cuda), torch.device("cuda"))
        pred = {k: t.to(dev).contiguous() for k, t in pred.items()}
        gt = {k: t.to(dev).contiguous() for k, t in gt.items()}
        if joint_regressor is not None:
            reg = joint_regressor.to(dev)
            pred["joints"] = torch.einsum("kv,fpvc->fpkc", reg, pred["verts"]).contiguous()
            gt["joints"] = torch.einsum("kv,fpvc->fpkc", reg, gt["verts"]).contiguous()
        us, M = float(unit_scale), F * P
        out = {"n_items": M}
        pr = gr = None
        if both_joints:
            pr, gr = pred["joints"][:, :, int(root)].reshape(M, 3).contiguous(), gt["joints"][:, :, int(root)].reshape(M, 3).contiguous()

        def score(kind, names, roots):
            e = hip.pose_errors(pred[kind].reshape(M, -1, 3), gt[kind].reshape(M, -1, 3), *roots).cpu().numpy()
            for col, key in zip((1, 0, 2), names):
                if key is not None:
                    out[key] = (e[:, col] * us).reshape(F, P)
                    out["mean_" + key] = _mean(out[key])
            out["n_left_out_" + kind] = int((e[:, 3] == 1).sum())
            out["n_degenerate_" + kind] = int((e[:, 3] == 2).sum())
        if both_joints:
            score("joints", ("mpjpe", "mpjpe_global", "pa_mpjpe"), (pr, gr))
        if both_verts:
            score("verts", ("mve" if both_joints else None, "mve_global", "pa_mve"), (pr, gr) if both_joints else ())

        # ---- depth relations of the roots
        if both_joints:
            def depth(rootpos):
                r = rootpos.reshape(F, P, 3)
                if view is None:
                    return r[:, :, 2]
                w = view.to(dev).float()
                w = w[None].expand(F, 3, 4) if w.dim() == 2 else w
                return (r * w[:, None, 2, :3]).sum(-1) + w[:, None, 2, 3]
            rp, okp = depth_relations(depth(pr), depth_threshold, us)
            rg, okg = depth_relations(depth(gr), depth_threshold, us)
            ok = okp & okg
            hit, cnt = ((rp == rg) & ok).sum(1).cpu().numpy().astype(np.float64), ok.sum(1).cpu().numpy().astype(np.float64)
            per = np.full(F, np.nan)
            np.divide(hit, cnt, out=per, where=cnt > 0)
            out.update(pcdr=float(hit.sum() / cnt.sum()) if cnt.sum() > 0 else math.nan, pcdr_per_frame=per,
                       n_depth_pairs=int(cnt.sum()))

        # ---- contact distance
        if contacts is not None:
            order = np.argsort(contacts["frame"], kind="stable")
            corr = np.stack([contacts[k][order] for k in ("frame", "person_a", "vertex", "person_b", "face")], 1).astype(np.int32)
            start = np.searchsorted(contacts["frame"][order], np.arange(F + 1)).astype(np.int32)
            args = (torch.from_numpy(faces).to(dev), torch.from_numpy(np.ascontiguousarray(corr)).to(dev).reshape(-1, 5),
                    torch.from_numpy(np.ascontiguousarray(contacts["bary"][order])).to(dev).reshape(-1, 3), torch.from_numpy(start).to(dev))
            for key, bodies in (("cd", pred["verts"]), ("cd_gt", gt["verts"])):
                r = hip.contact_distance(bodies, *args).cpu().numpy()
                out[key], out[key + "_per_frame"] = float(r[0] * us), r[2:2 + F] * us
            out.update(n_contacts=int(corr.shape[0]), n_contacts_per_frame=r[2 + F:].astype(np.int64))
    return out
