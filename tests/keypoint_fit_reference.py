"""Float64 torch-CPU restatement of the keypoint-fit objective and of its Adam loop (multiply_amd/keypoint_fit.py,
csrc/keypoint_fit.hip): the body is oracle.multiply_oracle.smpl_server_forward in double precision under autograd (scale 1,
absolute transforms), the loss is preprocessing/loss.py's spelled out, the optimiser is torch.optim.Adam's single-tensor step
written by hand (tests/test_keypoint_fit_cpu.py pins it on torch.optim.Adam and the formulas on hand-computed values before
anything on the device is compared against this file).  Not a test."""
import copy

import numpy as np
import torch

from oracle import multiply_oracle as O

REF = dict(rho=100.0, w_2d=1e-2, w_t=6.0, w_p=5.0)


def tables64(smpl_tables):
    """the oracle's SMPL tables (fp32 values) upcast to float64"""
    T = copy.copy(O.SMPLTables(smpl_tables))
    for k, v in vars(T).items():
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(T, k, v.double())
    return T


def reduced_tables(T, kmap):
    """The same body at the map's support vertices only, so that a 150-step loop takes seconds: the rest joints are LINEAR in the
    vertices (J = J_regressor (v_template + shapedirs betas) = J_regressor v_template + (J_regressor shapedirs) betas), so 24
    pseudo-vertices that carry those two products, regressed by the identity, give the oracle the same joints; the support
    vertices follow with their own rows.  Returns (tables, map) for keypoints3d; test_keypoint_fit_cpu.py compares the two."""
    sv = torch.as_tensor(kmap.support)
    R = copy.copy(T)
    S = len(kmap.support)
    R.v_template = torch.cat([T.J_regressor @ T.v_template, T.v_template[sv]], 0)
    R.shapedirs = torch.cat([torch.einsum("jv,vkl->jkl", T.J_regressor, T.shapedirs), T.shapedirs[sv]], 0)
    R.posedirs = torch.cat([torch.zeros(207, 72, dtype=torch.float64), T.posedirs.reshape(207, -1, 3)[:, sv].reshape(207, 3 * S)], 1)
    R.J_regressor = torch.cat([torch.eye(24, dtype=torch.float64), torch.zeros(24, S, dtype=torch.float64)], 1)
    R.lbs_weights = torch.cat([torch.zeros(24, 24, dtype=torch.float64), T.lbs_weights[sv]], 0)
    return R, _Shifted(kmap)


class _Shifted:
    """kmap over reduced tables: support vertex i is vertex 24 + i"""

    def __init__(self, kmap):
        self.support, self._dense = np.arange(24, 24 + len(kmap.support)), kmap.dense()

    def dense(self):
        return self._dense


class _Double:
    """the oracle's constant tensors follow the default dtype"""

    def __enter__(self):
        self.dt = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *a):
        torch.set_default_dtype(self.dt)


def rot6d(thetas):
    """(24, 6): the first two columns of each joint's rotation matrix, row-major (rotation.py axis_to_rot6D)"""
    return O.rodrigues(thetas.reshape(-1, 3))[:, :, :2].reshape(-1, 6)


def gmof(r, rho):
    """preprocessing_utils.py GMoF.forward"""
    return rho ** 2 * (r ** 2 / (r ** 2 + rho ** 2))


def project(X, cam):
    """X (K, 3), cam (16,) = fx, fy, cx, cy, E (3, 4) -> uv (K, 2), z_c (K,)"""
    E = cam[4:].reshape(3, 4)
    xc = X @ E[:, :3].T + E[:, 3]
    return torch.stack([cam[0] * xc[:, 0] / xc[:, 2] + cam[2], cam[1] * xc[:, 1] / xc[:, 2] + cam[3]], 1), xc[:, 2]


def keypoints3d(T, kmap, p):
    """the K keypoints (K, 3) of parameters p (85,) = [transl, thetas, betas]"""
    out = O.smpl_server_forward(T, torch.tensor(1.0, dtype=torch.float64), p[0:3], p[3:75], p[75:85])
    src = torch.cat([out["smpl_jnts"], out["smpl_verts"][torch.as_tensor(kmap.support)]], 0)
    return torch.as_tensor(kmap.dense()) @ src


def objective(T, kmap, p, targets, c, cam, prev=None, rho=REF["rho"], w_2d=REF["w_2d"], w_t=REF["w_t"], w_p=REF["w_p"]):
    """terms (3,) = [L2d, Lt, w_2d L2d + w_t Lt] (differentiable in p), proj (K, 2), flag.  All arguments double tensors."""
    with _Double():
        uv, z = project(keypoints3d(T, kmap, p), cam)
        ok = z > 0
        g = gmof(targets - torch.where(ok[:, None], uv, targets), rho)          # a keypoint behind the camera contributes nothing
        l2d = (c[:, None] * g * ok[:, None]).sum()
        if prev is None:
            lt = torch.zeros((), dtype=torch.float64)
        else:
            lt = w_p * ((rot6d(p[3:75]) - rot6d(prev[3:75]).detach()) ** 2).mean() + ((p[0:3] - prev[0:3]) ** 2).mean()
        return torch.stack([l2d, lt, w_2d * l2d + w_t * lt]), torch.where(ok[:, None], uv, torch.zeros_like(uv)).detach(), int((~ok).any())


def objective_and_grad(T, kmap, p, targets, c, cam, prev=None, **w):
    p = p.detach().double().clone().requires_grad_(True)
    terms, proj, flag = objective(T, kmap, p, targets, c, cam, prev, **w)
    g, = torch.autograd.grad(terms[2], p, allow_unused=True)
    return terms.detach(), (torch.zeros_like(p) if g is None else g), proj, flag


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor step t (1-based) with per-entry lr: returns the new (p, m, v)"""
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    step = lr / (1 - beta1 ** t)
    denom = v.sqrt() / np.sqrt(1 - beta2 ** t) + eps
    return p - step * (m / denom), m, v


def lr_row(lr):
    lt, lp, lb = (lr,) * 3 if np.ndim(lr) == 0 else lr
    return torch.tensor([float(lt)] * 3 + [float(lp)] * 72 + [float(lb)] * 10, dtype=torch.float64)


def fit(T, kmap, start, targets, c, cam, prev=None, iters=150, lr=1e-3, **w):
    """the Adam loop on one row: final parameters (85,), history (iters, 3) of the terms before each step"""
    p = start.detach().double().clone()
    m, v, lrs = torch.zeros_like(p), torch.zeros_like(p), lr_row(lr)
    hist = torch.zeros(iters, 3, dtype=torch.float64)
    for it in range(iters):
        terms, g, _, _ = objective_and_grad(T, kmap, p, targets, c, cam, prev, **w)
        hist[it] = terms
        p, m, v = adam_step(p, g, m, v, it + 1, lrs)
    return p, hist
