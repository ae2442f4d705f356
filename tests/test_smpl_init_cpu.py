"""The mesh fit (multiply_amd/smpl_init.py, csrc/fit.hip) without a GPU: the C ABI of the three kernels, the closedness check, the
file format, and the float64 restatement of the sampling map and of the objective -- which tests/test_smpl_init_gpu.py holds the
kernels to -- against cases computed by hand."""
import ast
import os

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_ARGS = {"mp_fit_area_cdf": 6, "mp_fit_sample": 17, "mp_fit_loss": 15}       # include/multiply_hip.h


# ------------------------------------------------------------------------------------------------ float64 restatement
def icosphere(n=2, radius=0.5):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
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
    return torch.tensor(v * radius, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def ref_area_cdf(face_verts):
    """(F,3,3) -> area, unit normal, inclusive area CDF normalised to 1 (float64); a cross product shorter than 1e-12: area 0"""
    fv = face_verts.double()
    c = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1)
    l = c.norm(dim=1)
    ok = l >= 1e-12
    area = torch.where(ok, 0.5 * l, torch.zeros_like(l))
    normal = torch.where(ok[:, None], c / l.clamp_min(1e-300)[:, None], torch.zeros_like(c))
    cdf = torch.cumsum(area, 0) / area.sum()
    return area, normal, cdf


def ref_sample(face_verts, normal, cdf, u_surf, z_near, sigma, u_box, box):
    """the sampling map: face = first f with cdf[f] > u0; barycentrics (1 - r, r (1 - u2), r u2), r = sqrt(u1); volume point j <
    n_near = surface point (j mod n_s) + sigma z_j, the others uniform in box (2,3)"""
    fv, u = face_verts.double(), u_surf.double()
    n_s = u.shape[0]
    face = torch.searchsorted(cdf.contiguous(), u[:, 0].contiguous(), right=True).clamp_max(cdf.shape[0] - 1)
    r = u[:, 1].sqrt()
    b = torch.stack([1 - r, r * (1 - u[:, 2]), r * u[:, 2]], 1)
    pts = (b[:, :, None] * fv[face]).sum(1)
    near = pts[torch.arange(z_near.shape[0]) % max(n_s, 1)] + sigma * z_near.double() if z_near.shape[0] else pts[:0]
    bx = box.double()
    vol = torch.cat([near, bx[0] + u_box.double() * (bx[1] - bx[0])])
    return pts, normal[face], face, vol


def _norm(v):
    """2-norm over the last axis with a ZERO subgradient below 1e-12"""
    n2 = (v * v).sum(-1)
    ok = n2 >= 1e-24
    return torch.where(ok, torch.where(ok, n2, torch.ones_like(n2)).sqrt(), n2.detach().sqrt())


def ref_loss(sdf, grad, normals, dist, weights, truncation=0.0):
    """terms (5,) = total, surface, normal, distance, eikonal of the fit's objective; the first len(normals) points are the
    surface points, the other len(dist) the volume points.  Differentiable in sdf and grad (torch autograd)."""
    n_s, n_v = normals.shape[0], dist.shape[0]
    zero = sdf.new_zeros(())
    fs, fv = sdf[:n_s], sdf[n_s:n_s + n_v]
    surface = fs.abs().mean() if n_s else zero
    normal = _norm(grad[:n_s] - normals).mean() if n_s else zero
    if truncation > 0:
        fv, dist = fv.clamp(-truncation, truncation), dist.clamp(-truncation, truncation)
    distance = (fv - dist).abs().mean() if n_v else zero
    eik = ((_norm(grad) - 1.0) ** 2).mean() if n_s + n_v else zero
    total = weights[0] * surface + weights[1] * normal + weights[2] * distance + weights[3] * eik
    return torch.stack([total, surface, normal, distance, eik])


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_binding_calls_the_three_entry_points():
    from multiply_amd import hip
    protos = hip.header_prototypes()
    for name, n in FIT_ARGS.items():
        assert name in protos, name
        assert len(protos[name][1]) == n and protos[name][0] is not None            # int status
    # hip.py calls exactly these names with as many arguments as the header declares
    tree = ast.parse(open(os.path.join(REPO, "multiply_amd", "hip.py")).read())
    calls = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("mp_fit_"):
            calls[node.func.attr] = len(node.args)
    assert calls == FIT_ARGS
    for fn in ("fit_area_cdf", "fit_sample", "fit_loss"):
        assert callable(getattr(hip, fn))


def test_library_exports_the_fit_kernels():
    import ctypes
    from multiply_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    assert all(hasattr(lib, n) for n in FIT_ARGS)


# ------------------------------------------------------------------------------------------------ closedness, file format
def test_closedness_check():
    from multiply_amd import smpl_init as S
    from multiply_amd.synthetic import make_smpl_tables
    v, f = icosphere(2)
    assert S.mesh_is_closed(f) and S.mesh_is_closed(f.numpy())
    assert not S.mesh_is_closed(f[:-1])                                   # one face removed: three edges with a single face
    assert not S.mesh_is_closed(make_smpl_tables(0)["f"])                 # the synthetic tables' placeholder triangles
    with pytest.raises(ValueError, match="exactly two faces"):
        S.require_closed(make_smpl_tables(0)["f"])
    S.require_closed(f)


def test_save_smpl_init_round_trip(tmp_path):
    from multiply_amd import smpl_init as S
    from tests.util import seeded_networks
    m, _ = seeded_networks(1, 0)
    net = m.foreground_implicit_network_list[0]
    path = S.save_smpl_init(net, str(tmp_path / "smpl_init.pth"))
    state = torch.load(path, map_location="cpu")
    assert list(state.keys()) == ["model_state_dict"]
    sd = state["model_state_dict"]
    assert set(sd.keys()) == set(net.state_dict().keys())
    m2, _ = seeded_networks(1, 1)
    other = m2.foreground_implicit_network_list[0]
    res = other.load_state_dict(sd, strict=False)                         # what the loader does (multiply.py:117-119)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in net.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k


def test_config_defaults():
    from multiply_amd.smpl_init import FitConfig
    c = FitConfig()
    assert (c.n_surface, c.n_volume, c.near_fraction, c.sigma_local, c.box_inflate) == (8192, 8192, 0.5, 0.05, 0.2)
    assert c.weights == (1.0, 1.0, 1.0, 0.1) and c.truncation == 0 and c.lr == 5e-4 and c.steps == 2000 and c.seed == 0
    assert c.n_near == 4096


# ------------------------------------------------------------------------------------------------ restatement vs hand-computed
def test_sampling_map_one_triangle():
    fv = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    area, normal, cdf = ref_area_cdf(fv)
    assert area.tolist() == [0.5] and normal.tolist() == [[0.0, 0.0, 1.0]] and cdf.tolist() == [1.0]
    u = torch.tensor([[0.3, 0.25, 0.5], [0.9, 1.0, 0.0], [0.0, 0.0, 0.7]])
    z = torch.tensor([[1.0, -2.0, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    box = torch.tensor([[-1.0, -2.0, -3.0], [1.0, 2.0, 3.0]])
    pts, nrm, face, vol = ref_sample(fv, normal, cdf, u, z, 0.1, torch.tensor([[0.5, 0.25, 1.0]]), box)
    # r = 0.5: (b0, b1, b2) = (0.5, 0.25, 0.25); r = 1, u2 = 0: vertex B; r = 0: vertex A
    assert torch.allclose(pts, torch.tensor([[0.25, 0.25, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64), atol=1e-15)
    assert face.tolist() == [0, 0, 0] and nrm.tolist() == [[0.0, 0.0, 1.0]] * 3
    want_vol = torch.tensor([[0.35, 0.05, 0.05], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.25, 0.35, 0.0], [0.0, -1.0, 3.0]], dtype=torch.float64)
    assert torch.allclose(vol, want_vol, atol=1e-7)                       # (0.1 is a float32 constant here)


def test_sampling_map_skips_degenerate_faces():
    # areas 0.5, 0 (repeated vertex), 1.5: the CDF is [0.25, 0.25, 1]
    fv = torch.tensor([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.0, 0, 0], [0, 0, 0], [0, 1, 0]], [[0.0, 0, 0], [3, 0, 0], [0, 1, 0]]])
    area, normal, cdf = ref_area_cdf(fv)
    assert area.tolist() == [0.5, 0.0, 1.5] and cdf.tolist() == [0.25, 0.25, 1.0] and normal[1].tolist() == [0.0, 0.0, 0.0]
    u = torch.tensor([[0.0, 0.5, 0.5], [0.2499, 0.5, 0.5], [0.25, 0.5, 0.5], [0.9999, 0.5, 0.5]])
    face = ref_sample(fv, normal, cdf, u, torch.zeros(0, 3), 0.0, torch.zeros(0, 3), torch.zeros(2, 3))[2]
    assert face.tolist() == [0, 0, 2, 2]


def _hand_case():
    sdf = torch.tensor([0.1, -0.3, 0.5, -0.2], dtype=torch.float64)
    grad = torch.tensor([[0.0, 0, 1], [0, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=torch.float64)
    normals = torch.tensor([[0.0, 0, 1], [0, 1, 0]], dtype=torch.float64)
    dist = torch.tensor([0.2, -0.2], dtype=torch.float64)
    return sdf, grad, normals, dist


def test_loss_hand_computed_truncation_off_and_on():
    sdf, grad, normals, dist = _hand_case()
    w = (1.0, 1.0, 1.0, 0.1)
    # surface (0.1 + 0.3) / 2; normal (0 + 1) / 2; distance (0.3 + 0) / 2; eikonal (0 + 1 + 1 + 0) / 4
    t = ref_loss(sdf, grad, normals, dist, w)
    assert torch.allclose(t, torch.tensor([0.2 + 0.5 + 0.15 + 0.05, 0.2, 0.5, 0.15, 0.5], dtype=torch.float64), atol=1e-15)
    # truncation 0.3: clamp(0.5) = 0.3 against 0.2 -> (0.1 + 0) / 2
    t = ref_loss(sdf, grad, normals, dist, w, truncation=0.3)
    assert torch.allclose(t, torch.tensor([0.2 + 0.5 + 0.05 + 0.05, 0.2, 0.5, 0.05, 0.5], dtype=torch.float64), atol=1e-15)


def test_loss_gradients_hand_computed_incl_zero_norm():
    sdf, grad, normals, dist = _hand_case()
    w = (1.0, 2.0, 3.0, 0.1)
    for tau, d_f2 in ((0.0, 1.5), (0.3, 0.0)):                            # f = 0.5 lies outside the clamp's range: no gradient
        s, g = sdf.clone().requires_grad_(True), grad.clone().requires_grad_(True)
        ref_loss(s, g, normals, dist, w, tau)[0].backward()
        # d sdf: surface sign / 2; distance 3 sign(0.3) / 2, and |0| contributes 0
        assert torch.allclose(s.grad, torch.tensor([0.5, -0.5, d_f2, 0.0], dtype=torch.float64), atol=1e-15)
        # d grad: point 0: residual 0 and |grad| = 1 -> 0; point 1: ZERO-norm gradient -> the eikonal term contributes 0, the normal
        # term 2 (0 - n) / |.| / 2; point 2: eikonal 0.1 * 2 (2 - 1) / 4 along x; point 3: |grad| = 1 -> 0
        want = torch.tensor([[0.0, 0, 0], [0, -1.0, 0], [0.05, 0, 0], [0, 0, 0]], dtype=torch.float64)
        assert torch.allclose(g.grad, want, atol=1e-15) and torch.isfinite(g.grad).all()


def test_loss_empty_sets_are_zero_not_nan():
    sdf, grad, normals, dist = _hand_case()
    w = (1.0, 1.0, 1.0, 0.1)
    t = ref_loss(sdf[:2], grad[:2], normals, dist[:0], w)                 # empty V
    assert torch.allclose(t, torch.tensor([0.2 + 0.5 + 0.0 + 0.05, 0.2, 0.5, 0.0, 0.5], dtype=torch.float64), atol=1e-15)
    t = ref_loss(sdf[2:], grad[2:], normals[:0], dist, w)                 # empty S
    assert torch.allclose(t, torch.tensor([0.15 + 0.05, 0.0, 0.0, 0.15, 0.5], dtype=torch.float64), atol=1e-15)
    assert torch.equal(ref_loss(sdf[:0], grad[:0], normals[:0], dist[:0], w), torch.zeros(5, dtype=torch.float64))
