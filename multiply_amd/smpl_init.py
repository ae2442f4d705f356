"""Fit a foreground ImplicitNet to a closed triangle mesh on the device and write the `smpl_init` file the model loads.

The reference never trains from the geometric sphere: it warm-starts every foreground ImplicitNet from
`outputs/smpl_init_male_256.pth`, a network pre-fitted to the canonical SMPL surface (lib/model/multiply.py:102-108).  That file
is an asset outside its tree and so is the recipe that made it; this module is the producer.  The objective is the published
one of implicit geometric regularisation (Gropp et al., "Implicit Geometric Regularization for Learning Shapes", ICML 2020)
with a supervised distance term, since the exact signed distance to the mesh is available (mp_mesh_signed_distance):

    surface   mean_S |f|                      f = the network's sdf, S = area-uniform points on the mesh
    normal    mean_S |grad f - n|_2           n = the face normal
    distance  mean_V |f - d|                  V = points near the surface and uniform in a box, d = exact signed distance
    eikonal   mean_{S u V} (|grad f|_2 - 1)^2

One step = torch draws the random numbers (seeded generator) -> mp_fit_sample -> mp_mesh_signed_distance -> the layer-fused value +
gradient sweep of the network (train.ImplicitTrainFused) -> mp_fit_loss -> the sweep's adjoint -> fused Adam.  Nothing in a step
waits for the device unless `log_every` asks for the terms.
"""
import dataclasses
import time

import numpy as np
import torch

from . import hip

TERM_NAMES = ("total", "surface", "normal", "distance", "eikonal")


@dataclasses.dataclass
class FitConfig:
    """Every setting of the fit (settings, not measurements)."""
    n_surface: int = 8192
    n_volume: int = 8192
    near_fraction: float = 0.5        # share of the volume points that are surface points + sigma_local * N(0, 1)
    sigma_local: float = 0.05
    box: object = None                # (2, 3) lo / hi of the uniform volume points; None: the mesh's bounding box inflated by box_inflate
    box_inflate: float = 0.2
    w_surface: float = 1.0
    w_normal: float = 1.0
    w_distance: float = 1.0
    w_eikonal: float = 0.1
    truncation: float = 0.0           # > 0: the distance term compares clamp(f) with clamp(d) on [-truncation, truncation]
    lr: float = 5e-4
    steps: int = 2000
    seed: int = 0

    @property
    def n_near(self):
        return 0 if self.n_surface == 0 else int(round(self.n_volume * self.near_fraction))

    @property
    def weights(self):
        return (self.w_surface, self.w_normal, self.w_distance, self.w_eikonal)


@dataclasses.dataclass
class FitRecord:
    """What a fit did: the logged terms [(step, {name: value})], the settings that identify it and its speed."""
    steps: int
    seed: int
    n_faces: int
    ms_per_step: float
    terms: list = dataclasses.field(default_factory=list)

    def __str__(self):
        last = ", ".join(f"{k} {v:.4e}" for k, v in self.terms[-1][1].items()) if self.terms else "no terms logged"
        return (f"fit: {self.steps} steps, seed {self.seed}, {self.n_faces} faces, {self.ms_per_step:.2f} ms / step; "
                f"last logged: {last}")


def mesh_is_closed(faces):
    """every undirected edge of the triangle list is shared by exactly two faces (host side)"""
    f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).astype(np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return False
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1], return_counts=True)
    return bool((counts == 2).all())


def require_closed(faces, what="the mesh"):
    if not mesh_is_closed(faces):
        raise ValueError(f"{what} is not a closed surface: every undirected edge must be shared by exactly two faces (a signed "
                         f"distance needs an inside).  The synthetic SMPL tables' `f` is a placeholder, not a surface: fit to "
                         f"synthetic.closed_body_mesh(server) instead")


def make_draws(cfg, gen, device):
    """the random numbers of one step, in the order the fit consumes them: u_surf (n_s,3), z_near (n_near,3), u_box (rest,3)"""
    n_s, n_near = cfg.n_surface, cfg.n_near
    u_surf = torch.rand(n_s, 3, generator=gen, device=device)
    z_near = torch.randn(n_near, 3, generator=gen, device=device)
    u_box = torch.rand(cfg.n_volume - n_near, 3, generator=gen, device=device)
    return u_surf, z_near, u_box


def fit_box(cfg, verts, device):
    if cfg.box is not None:
        return torch.as_tensor(np.asarray(cfg.box, dtype=np.float32)).reshape(2, 3).to(device).contiguous()
    lo, hi = verts.min(dim=0).values, verts.max(dim=0).values
    return torch.stack([lo - cfg.box_inflate, hi + cfg.box_inflate]).contiguous()


def _mesh_tensors(verts, faces, device):
    v = torch.as_tensor(np.asarray(verts) if not torch.is_tensor(verts) else verts).to(device).float().reshape(-1, 3)
    f = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device).long().reshape(-1, 3)
    return v, f


class MeshTarget:
    """device-side tables of the mesh a fit samples: face vertices, areas, normals, the area CDF"""

    def __init__(self, verts, faces, device="cuda", mesh_index_mode=None):
        self.verts, self.faces = _mesh_tensors(verts, faces, device)
        self.face_verts = self.verts[self.faces].contiguous()                 # (F,3,3), the layout of mesh_face_vertices_list
        self.area, self.normal, self.cdf = hip.fit_area_cdf(self.face_verts)
        self.n_faces = self.faces.shape[0]
        # the distances of every step's volume points go through a face index ('auto': a closed mesh of hip.MESH_INDEX_MIN_FACES
        # faces or more; the fit itself refuses a mesh that is not closed)
        self.index = hip.MeshIndex(self.face_verts) if hip.mesh_index_wanted(mesh_index_mode, self.n_faces, self.faces) else None


def fit_step_points(target, cfg, box, draws, out=None):
    """mp_fit_sample + mp_mesh_signed_distance: points (n_s + n_v,3), surface normals, face ids, exact distances of the volume points"""
    u_surf, z_near, u_box = draws
    pts, nrm, fid = hip.fit_sample(target.face_verts, target.normal, target.cdf, u_surf, z_near, cfg.sigma_local, u_box, box, out)
    dist = hip.mesh_signed_distance(pts[cfg.n_surface:], target.face_verts, index=target.index)
    return pts, nrm, fid, dist


def fit_implicit_net(net, verts, faces, cond=None, cfg=None, log_every=0, mesh_index_mode=None):
    """Fits `net` (a foreground ImplicitNet on the device) to the CLOSED triangle mesh (verts (V,3), faces (F,3): device tensors or
    numpy, canonical space) and returns a FitRecord.  The parameters are updated in place.

    cond: the pose conditioning (69,) the network sees during the fit; None = the all-zero vector.  With zeros the conditioning
    columns of layer 0 multiply zeros: they receive NO gradient and keep their initial values (the geometric initialisation
    sets them to zero, so the fitted network starts pose-independent, like a network fitted without conditioning).

    mesh_index_mode: 'auto' | 'index' | 'brute' for the exact distances (None = hip.MESH_INDEX_MODE; same values either way).

    log_every > 0: the five terms are read back (a host synchronisation) at step 1, every log_every steps and at the last."""
    from . import train as T
    cfg = FitConfig() if cfg is None else cfg
    if not T.fused_sdf_supported(net):
        raise NotImplementedError("fit_implicit_net runs on the layer-fused training kernels (csrc/tfuse.hip), which are specialised "
                                  "for the shipped foreground ImplicitNet: d_in 3, multires 6, 8 hidden layers of 256, skip_in [4], "
                                  "cond_dim 69, 257 outputs")
    hip.require_device()
    dev = next(net.parameters()).device
    require_closed(faces)
    target = MeshTarget(verts, faces, dev, mesh_index_mode)
    box = fit_box(cfg, target.verts, dev)
    cond = torch.zeros(69, dtype=torch.float32, device=dev) if cond is None else cond.detach().to(dev).float().reshape(-1).contiguous()
    gen = torch.Generator(device=dev).manual_seed(int(cfg.seed))
    n_s, n_v = cfg.n_surface, cfg.n_volume
    n = n_s + n_v
    params = None
    opt = None
    dfeat = torch.zeros(n, 256, dtype=torch.float32, device=dev)              # the features carry no objective
    pts_out = loss_out = None
    rec = FitRecord(steps=cfg.steps, seed=cfg.seed, n_faces=target.n_faces, ms_per_step=0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(1, cfg.steps + 1):
        pts, nrm, fid, dist = fit_step_points(target, cfg, box, make_draws(cfg, gen, dev), pts_out)
        pts_out = (pts, nrm, fid)
        ev = T.ImplicitTrainFused(net, pts, cond, p_cap=n)                    # one stash allocation for all steps
        loss_out = hip.fit_loss(ev.sdf, ev.grad, nrm, dist, cfg.weights, cfg.truncation, loss_out)
        terms, d_sdf, d_grad = loss_out
        ev.backward(dfeat, d_sdf, d_grad)
        if params is None:
            params = ev.params()
            opt = torch.optim.Adam(params, lr=cfg.lr, fused=True)
        for p, g in zip(params, ev.param_grads()):
            p.grad = g.reshape(p.shape)
        opt.step()
        if log_every and (step == 1 or step % log_every == 0 or step == cfg.steps):
            rec.terms.append((step, dict(zip(TERM_NAMES, terms.cpu().tolist()))))   # the host synchronisation log_every asks for
    torch.cuda.synchronize()
    rec.ms_per_step = (time.perf_counter() - t0) * 1e3 / max(cfg.steps, 1)
    for p in (params or []):
        p.grad = None
    # torch's fused Adam does not bump the parameters' version counters (hip.py: "_GENERATION"): forget every packed-weight cache,
    # as Multiply.train()/eval() does, so that the next inference call packs the fitted weights
    hip.invalidate_packed()
    return rec


def save_smpl_init(net, path):
    """writes {"model_state_dict": net.state_dict()}: what Multiply.__init__ (multiply.py:117-119) and the reference's
    load_state_dict(state["model_state_dict"], strict=False) read"""
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in net.state_dict().items()}}, path)
    return path


def heldout_error(net, verts, faces, cond=None, n_surface=4096, n_box=4096, seed=12345, box=None, box_inflate=0.2,
                  mesh_index_mode=None):
    """mean / max |sdf - exact signed distance| of the network on held-out points: n_surface area-uniform surface points (exact
    distance 0) and n_box points uniform in the fit's box.  The network runs through the near-fp32 training sweep (forward only).
    Returns {"surface_mean", "surface_max", "box_mean", "box_max"} (host floats; synchronises)."""
    from . import train as T
    dev = next(net.parameters()).device
    target = MeshTarget(verts, faces, dev, mesh_index_mode)
    cfg = FitConfig(n_surface=n_surface, n_volume=n_box, near_fraction=0.0, box=box, box_inflate=box_inflate)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    pts, _, _, dist = fit_step_points(target, cfg, fit_box(cfg, target.verts, dev), make_draws(cfg, gen, dev))
    cond = torch.zeros(69, dtype=torch.float32, device=dev) if cond is None else cond.detach().to(dev).float().reshape(-1).contiguous()
    with torch.no_grad():
        f = T.ImplicitTrainFused(net, pts, cond).sdf[:pts.shape[0]]
    es, eb = f[:n_surface].abs(), (f[n_surface:] - dist).abs()
    return {"surface_mean": float(es.mean()), "surface_max": float(es.max()), "box_mean": float(eb.mean()), "box_max": float(eb.max())}


def fit_smpl_init(model_or_opt, path, person=0, mesh=None, cfg=None, log_every=0):
    """Fits person's foreground ImplicitNet and writes the smpl_init file to `path`; returns (net, FitRecord).

    model_or_opt: a Multiply model (its network is fitted in place) or a model config (a fresh ImplicitNet is built from
    opt.implicit_network on the device; `mesh` is then required).  mesh = (verts, faces), default the model's canonical mesh
    (mesh_v_cano_list[person], mesh_f_cano_list[person]): with real SMPL tables the canonical SMPL surface.  A mesh that is not
    closed is refused (the synthetic tables' `f` is a list of near-neighbour triangles, not a surface).  A model's
    mesh_index_mode applies to the fit's exact distances too."""
    mode = None
    if hasattr(model_or_opt, "foreground_implicit_network_list"):
        model = model_or_opt
        mode = model.mesh_index_mode
        net = model.foreground_implicit_network_list[person]
        if mesh is None:
            mesh = (model.mesh_v_cano_list[person].reshape(-1, 3), model.mesh_f_cano_list[person])
    else:
        from .networks import ImplicitNet
        if mesh is None:
            raise ValueError("fit_smpl_init(opt, ...) needs mesh=(verts, faces): a config has no canonical mesh")
        net = ImplicitNet(model_or_opt.implicit_network).to("cuda")
    verts, faces = mesh
    require_closed(faces, "the mesh to fit")
    rec = fit_implicit_net(net, verts, faces, cond=None, cfg=cfg, log_every=log_every, mesh_index_mode=mode)
    save_smpl_init(net, path)
    return net, rec
