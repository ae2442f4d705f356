"""float64 references, per-element error bounds and input generators of the element-wise / small training kernels
(csrc/train.hip, mp_tr_*).  torch and numpy only: no GPU, no project imports.

Three statements of every kernel, all taking the float32 inputs the kernel gets (a dict, see the case builders below):

  REFS[name]   the DEFINITION in float64.  Adjoints come from torch.autograd on that definition (the softplus second-order
               term, the double normalise of shade_in, the inverse of warp_bwd and the transmittance of bg_comp are written
               by hand once, in the kernel; autograd is the independent statement of them).
  TREES[name]  the kernel's own EXPRESSION TREE, operation by operation, written once over a small arithmetic interface and
               evaluated two ways: on float32 CPU tensors (the "emulation": the same tree in the host's float32), and on EB
               values (below), which carry the float64 value together with a first-order bound of the rounding error.
  bound        EB's error of the tree + FLOOR.  Model: every arithmetic operation rounds once, fl(x) = x (1 + d) + h with
               |d| <= u = 2^-24 and |h| <= 2^-150 (half a denormal step); every call of expf, log1pf, sinf, cosf, sqrtf and
               every division is allowed U_F ulps, |d| <= U_F u; errors of the operands propagate with the partial
               derivatives of the operation (first order).  The amplifications follow from that and need no special case:
               the rounding of t = 100 z enters expf times |t|; 1 - d1 near d1 = 1 keeps d1's absolute error, which
               100 d1 (1 - d1) then multiplies by 100; f cos(f x) carries f times cosf's error; a sum of n terms is charged
               (n - 1) u sum|terms| whatever its order; warp_bwd's cofactor inverse divides by det R, so every entry of
               dtfs is charged sum|contributions| times the conditioning of R.  Multiplications by a power of two (x 2^k)
               are exact and charged nothing; constants that float32 does not hold (0.01f, 1e-12f, 1e-6f) are charged u.
               FLOOR, the smallest normal float32, is added once per element for results that underflow on the device.

Nothing here is fitted to what the kernels return: U_F = 1, and the only measured quantity is how close the host's float32
evaluation of the same tree comes to the bound (cpu_ratio): tests/tolerances_train_elementwise.py turns that into the limit.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
ETA = 2.0 ** -150
FLOOR = 2.0 ** -126
U_F = 1.0
NJ = 24
Z8_LD = 257
PREACT_RMS = 0.15        # RMS of trained hidden pre-activations: tests/weight_regimes.py (_train_implicit, z_rms)


def f32(v):
    """a Python float that float32 holds exactly (scalar kernel arguments)"""
    return float(np.float32(v))


# ================================================================================================== error-bounded values
class EB:
    """float64 value v of an expression and a bound e of |its float32 evaluation - v| (model: the module's docstring)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @staticmethod
    def lift(x):
        if isinstance(x, EB):
            return x
        if isinstance(x, torch.Tensor):
            return EB(x.double())
        return EB(torch.tensor(float(x), dtype=torch.float64))

    @staticmethod
    def _r(v, e, k=1.0):
        return EB(v, e + k * U * v.abs() + ETA)

    def __add__(a, b):
        b = EB.lift(b)
        return EB._r(a.v + b.v, a.e + b.e)
    __radd__ = __add__

    def __sub__(a, b):
        b = EB.lift(b)
        return EB._r(a.v - b.v, a.e + b.e)

    def __rsub__(a, b):
        return EB.lift(b) - a

    def __mul__(a, b):
        b = EB.lift(b)
        return EB._r(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e)
    __rmul__ = __mul__

    def __truediv__(a, b):
        b = EB.lift(b)
        q = a.v / b.v
        return EB._r(q, a.e / b.v.abs() + q.abs() * b.e / b.v.abs(), U_F)

    def __rtruediv__(a, b):
        return EB.lift(b) / a

    def __neg__(a):
        return EB(-a.v, a.e)

    def __getitem__(a, i):
        return EB(a.v[i], a.e[i])

    @property
    def shape(a):
        return a.v.shape

    def x2(a, f):                                   # times a power of two: exact
        return EB(a.v * f, a.e * abs(f))

    def abs(a):
        return EB(a.v.abs(), a.e)

    def exp(a):
        v = a.v.exp()
        return EB._r(v, v * a.e, U_F)

    def log1p(a):
        return EB._r(a.v.log1p(), a.e / (1.0 + a.v).abs(), U_F)

    def sin(a):
        return EB._r(a.v.sin(), a.v.cos().abs() * a.e, U_F)

    def cos(a):
        return EB._r(a.v.cos(), a.v.sin().abs() * a.e, U_F)

    def sqrt(a):
        v = a.v.sqrt()
        d = torch.where(v > 0, a.e / (2.0 * v.clamp_min(1e-300)), a.e.sqrt())
        return EB._r(v, d, U_F)

    def clamp_min(a, c):                            # fmaxf with a constant float32 holds to u
        return EB(a.v.clamp_min(c), a.e + U * abs(c))

    def sum(a, dim):
        n = a.v.shape[dim]
        return EB(a.v.sum(dim), a.e.sum(dim) + max(n - 1, 0) * U * a.v.abs().sum(dim) + ETA)

    def unsqueeze(a, d):
        return EB(a.v.unsqueeze(d), a.e.unsqueeze(d))


def _is_eb(*xs):
    return any(isinstance(x, EB) for x in xs)


def x2(x, f):
    return x.x2(f) if isinstance(x, EB) else x * f


def kc(like, c):
    """a constant that float32 rounds"""
    return EB(torch.tensor(c, dtype=torch.float64), torch.tensor(U * abs(c), dtype=torch.float64)) if isinstance(like, EB) else c


def gt(x, c):
    """x > (float) c, decided on the value"""
    return x.v > f32(c) if isinstance(x, EB) else x > c


def where(m, a, b):
    if _is_eb(a, b):
        a, b = EB.lift(a), EB.lift(b)
        return EB(torch.where(m, a.v, b.v), torch.where(m, a.e, b.e))
    if not isinstance(a, torch.Tensor):
        a = torch.full_like(b, a)
    if not isinstance(b, torch.Tensor):
        b = torch.full_like(a, b)
    return torch.where(m, a, b)


def cat(xs, dim=0):
    if _is_eb(*xs):
        xs = [EB.lift(x) for x in xs]
        return EB(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim))
    return torch.cat(xs, dim)


def stack(xs, dim=0):
    if _is_eb(*xs):
        xs = [EB.lift(x) for x in xs]
        return EB(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))
    return torch.stack(xs, dim)


def full(like, val):
    return EB(torch.full_like(like.v, val)) if isinstance(like, EB) else torch.full_like(like, val)


def tsum(x, dim):
    """a sum over `dim`: EB charges (n - 1) u sum|terms|; float32 tensors are added one after the other in float32 (torch's
    own sum picks an order by vector width and may accumulate wider, neither of which the kernels do)"""
    if isinstance(x, EB):
        return x.sum(dim)
    parts = x.unbind(dim)
    acc = parts[0].clone()
    for t in parts[1:]:
        acc = acc + t
    return acc


def take(x, idx):
    """rows idx of x (a gather: exact)"""
    return EB(x.v[idx], x.e[idx]) if isinstance(x, EB) else x[idx]


def with_input_rounding(x):
    """an input that is itself the float32 rounding of the reference's float64 value"""
    return EB(x.v, x.e + U * x.v.abs()) if isinstance(x, EB) else x


# ================================================================================================================ softplus
def softplus_hi(z32):
    """the kernel's branch: t = fl32(100 z) > 20"""
    assert z32.dtype == torch.float32
    return (z32 * 100.0) > 20.0


def branch_floats():
    """(largest float z with fl32(100 z) <= 20, the next float up, 0.2f)"""
    z = np.float32(0.2)
    while np.float32(z * np.float32(100.0)) <= np.float32(20.0):
        z = np.nextafter(z, np.float32(1.0))
    while np.float32(z * np.float32(100.0)) > np.float32(20.0):
        z = np.nextafter(z, np.float32(0.0))
    return float(z), float(np.nextafter(z, np.float32(1.0))), float(np.float32(0.2))


def softplus_values():
    lo, hi, z02 = branch_floats()
    return [0.0, 1e-6, -1e-6, 0.01, -0.01, 0.1, -0.1, lo, hi, z02, 0.5, -0.5, -0.9, -1.2, -10.0, 3.0]


def softplus_z(rows, C, seed):
    """Z [rows][C] float32: the edge values first (cyclically, so that every column phase of a float4 sees them), then a
    Gaussian fill at the scale of trained pre-activations"""
    g = torch.Generator().manual_seed(seed)
    z = (PREACT_RMS * torch.randn(rows * C, generator=g, dtype=torch.float64)).float()
    vals = torch.tensor(softplus_values(), dtype=torch.float64).float()
    n = min(z.numel(), 2 * vals.numel() + 3)
    z[:n] = vals.repeat(3)[:n]
    return z.view(rows, C)


def t_d012(z, hi):
    """softplus_d012 of train.hip"""
    t = z * 100.0
    e = where(hi, 0.0, t).exp()
    h = e.log1p() * kc(e, 0.01)
    d1 = e / (e + 1.0)
    d2 = (d1 * 100.0) * (1.0 - d1)
    return where(hi, z, h), where(hi, 1.0, d1), where(hi, 0.0, d2)


def r_softplus(z, hi):
    """nn.Softplus(beta=100, threshold=20) in float64 with the branch given (decided on the float32 product)"""
    zs = torch.where(hi, torch.zeros_like(z), z)
    return torch.where(hi, z, torch.log1p(torch.exp(100.0 * zs)) / 100.0)


def _grad(y, x, create_graph=True):
    if not y.requires_grad:
        return torch.zeros_like(x)
    g, = torch.autograd.grad(y, x, create_graph=create_graph, allow_unused=True)
    return torch.zeros_like(x) if g is None else g


def r_s012(z, hi, drop_d2=False):
    """(s, s', s'') of r_softplus by autograd; z must require grad.  drop_d2: the planted error of the CPU test."""
    s = r_softplus(z, hi)
    s1 = _grad(s.sum(), z)
    if drop_d2:
        s1 = s1.detach()
    s2 = _grad(s1.sum(), z)
    return s, s1, s2


def _leaf(x):
    return x.detach().clone().requires_grad_(True)


# ---- forward-mode softplus layer
def r_softplus_layer(Z, hi, P, scale, wrong_block=False):
    if P <= 0:
        return r_softplus(Z, hi) * scale
    Z0 = Z[:P]
    s = r_softplus(Z0, hi[:P])
    s1 = _grad(s.sum(), Z0) if Z.requires_grad else r_s012(_leaf(Z0), hi[:P])[1].detach()
    order = (2, 1, 3) if wrong_block else (1, 2, 3)
    return torch.cat([s * scale] + [s1 * Z[k * P:(k + 1) * P] * scale for k in order], 0)


def ref_softplus_fwd(x):
    return {"H": r_softplus_layer(x.Z, x.hi, x.P, x.scale).detach()}


def ref_softplus_bwd(x, drop_d2=False):
    Z = _leaf(x.Z)
    if x.P > 0:
        Z0 = Z[:x.P]
        s, s1, _ = r_s012(Z0, x.hi[:x.P], drop_d2)
        H = torch.cat([s * x.scale] + [s1 * Z[k * x.P:(k + 1) * x.P] * x.scale for k in (1, 2, 3)], 0)
    else:
        H = r_softplus(Z, x.hi) * x.scale
    return {"dZ": _grad((H * x.dH).sum(), Z, False).detach()}


def tree_softplus_fwd(x):
    P = x.P
    if P <= 0:
        return {"H": t_d012(x.Z, x.hi)[0] * x.scale}
    h, d1, _ = t_d012(x.Z[:P], x.hi[:P])
    return {"H": cat([h * x.scale] + [d1 * x.Z[k * P:(k + 1) * P] * x.scale for k in (1, 2, 3)], 0)}


def tree_softplus_bwd(x):
    P = x.P
    if P <= 0:
        _, d1, _ = t_d012(x.Z, x.hi)
        return {"dZ": d1 * x.dH * x.scale}
    _, d1, d2 = t_d012(x.Z[:P], x.hi[:P])
    dz = d1 * x.dH[:P] * x.scale
    tang = []
    for k in (1, 2, 3):
        dt = x.dH[k * P:(k + 1) * P] * x.scale
        dz = dz + d2 * x.Z[k * P:(k + 1) * P] * dt
        tang.append(d1 * dt)
    return {"dZ": cat([dz] + tang, 0)}


# ---- reverse-over-reverse passes
def _u(x):
    return x.U if x.U is not None else x.wrow.unsqueeze(0)


def ref_sigmul(x):
    _, s1, _ = r_s012(_leaf(x.Z), x.hi)
    return {"V": (s1 * _u(x) * x.scale).detach()}


def tree_sigmul(x):
    return {"V": t_d012(x.Z, x.hi)[1] * _u(x) * x.scale}


def ref_rev_adj(x):
    _, s1, _ = r_s012(_leaf(x.Z), x.hi)
    return {"dU": (s1 * x.dV).detach(), "dS": (_u(x) * x.uscale * x.dV).expand_as(x.dV).detach()}


def tree_rev_adj(x):
    d1 = t_d012(x.Z, x.hi)[1]
    dS = _u(x) * x.uscale * x.dV
    return {"dU": d1 * x.dV, "dS": dS}


def ref_dz(x):
    _, s1, s2 = r_s012(_leaf(x.Z), x.hi)
    return {"dZ": (s1 * x.dX * x.scale + s2 * x.dS).detach()}


def tree_dz(x):
    _, d1, d2 = t_d012(x.Z, x.hi)
    return {"dZ": d1 * x.dX * x.scale + d2 * x.dS}


def ref_rev_chain(x):
    """autograd, w.r.t. Z, of sum s(Z) scale dX + sum s'(Z) U uscale dV: what dz(Z, dX, scale, dS of rev_adj) must return"""
    Z = _leaf(x.Z)
    s, s1, _ = r_s012(Z, x.hi)
    return {"dZ": _grad((s * x.scale * x.dX).sum() + (s1 * _u(x) * x.uscale * x.dV).sum(), Z, False).detach()}


def tree_rev_chain(x):
    _, d1, d2 = t_d012(x.Z, x.hi)
    return {"dZ": d1 * x.dX * x.scale + d2 * (_u(x) * x.uscale * x.dV)}


# ======================================================================================================= Fourier features
def pe_width(D, L):
    return D + 2 * D * L


def pe_ref(x, L):
    """embedder layout: x, then per octave sin (D columns), cos (D columns)"""
    out = [x]
    for k in range(L):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]
    return torch.cat(out, -1)


def pe_tangents(x, L):
    """D tensors [P][NF]: d pe / d x_b by autograd (differentiable again); x must require grad"""
    out = pe_ref(x, L)
    cols = [_grad(out[:, c].sum(), x) for c in range(out.shape[1])]            # [P][D] each
    return out, [torch.stack([g[:, b] for g in cols], 1) for b in range(x.shape[1])]


def pe_rows(X, L, fwd):
    """value rows, and with fwd the D tangent blocks below them"""
    if not fwd:
        return pe_ref(X, L)
    out, tang = pe_tangents(X, L)
    return torch.cat([out] + tang, 0)


def ref_pe(x):
    return {"out": (pe_rows(_leaf(x.x), x.L, x.fwd) * x.scale).detach()}


def _sincos(X, L):
    res = []
    for k in range(L):
        a = x2(X, 2.0 ** k)
        res.append((2.0 ** k, a.sin(), a.cos()))
    return res


def tree_pe(x):
    X, D, L = x.x, x.x.shape[1], x.L
    sc = _sincos(X, L)
    cols = [X * x.scale]
    for f, s, c in sc:
        cols += [s * x.scale, c * x.scale]
    rows = [cat(cols, 1)]
    if x.fwd:
        zero, one = full(X[:, 0], 0.0), full(X[:, 0], x.scale)
        for b in range(D):
            cb = [zero] * pe_width(D, L)
            cb[b] = one
            for k, (f, s, c) in enumerate(sc):
                cb[D + 2 * D * k + b] = x2(c[:, b], f) * x.scale
                cb[D + 2 * D * k + D + b] = x2(-s[:, b], f) * x.scale
            rows.append(stack(cb, 1))
    return {"out": cat(rows, 0)}


def ref_pe_bwd(x):
    X = _leaf(x.x)
    return {"dx": (x.dx0 + _grad((pe_rows(X, x.L, x.fwd) * x.dIN).sum(), X, False)).detach()}


def tree_pe_bwd(x):
    X, D, L, P = x.x, x.x.shape[1], x.L, x.x.shape[0]
    sc = _sincos(X, L)
    dv, cols = x.dIN[:P], []
    for a in range(D):
        acc = dv[:, a]
        for k, (f, s, c) in enumerate(sc):
            i_s, i_c = D + 2 * D * k + a, D + 2 * D * k + D + a
            acc = acc + x2(c[:, a] * dv[:, i_s] - s[:, a] * dv[:, i_c], f)
            if x.fwd:
                dt = x.dIN[(a + 1) * P:(a + 2) * P]
                acc = acc - x2(s[:, a] * dt[:, i_s] + c[:, a] * dt[:, i_c], f * f)
        cols.append(x.dx0[:, a] + acc)
    return {"dx": stack(cols, 1)}


def ref_pe_grad_fwd(x):
    X = _leaf(x.x)
    return {"grad": _grad((pe_ref(X, x.L) * x.G).sum(), X, False).detach()}


def tree_pe_grad_fwd(x):
    sc = _sincos(x.x, x.L)
    cols = []
    for a in range(3):
        acc = x.G[:, a]
        for k, (f, s, c) in enumerate(sc):
            acc = acc + x2(c[:, a] * x.G[:, 3 + 6 * k + a] - s[:, a] * x.G[:, 3 + 6 * k + 3 + a], f)
        cols.append(acc)
    return {"grad": stack(cols, 1)}


def ref_pe_grad_bwd(x):
    X, G = _leaf(x.x), _leaf(x.G)
    grad = _grad((pe_ref(X, x.L) * G).sum(), X)
    loss = (grad * x.dgrad).sum()
    out = {"dG": _grad(loss, G, True).detach()}
    if x.dx0 is not None:
        out["dx"] = (x.dx0 + _grad(loss, X, False)).detach()
    return out


def tree_pe_grad_bwd(x):
    sc = _sincos(x.x, x.L)
    NF = pe_width(3, x.L)
    dg, dxs = [None] * NF, []
    for a in range(3):
        da = x.dgrad[:, a]
        dg[a] = da
        acc = full(da, 0.0)
        for k, (f, s, c) in enumerate(sc):
            dg[3 + 6 * k + a] = x2(da, f) * c[:, a]
            dg[3 + 6 * k + 3 + a] = x2(-da, f) * s[:, a]
            acc = acc - x2(da, f * f) * (s[:, a] * x.G[:, 3 + 6 * k + a] + c[:, a] * x.G[:, 3 + 6 * k + 3 + a])
        dxs.append(acc)
    out = {"dG": stack(dg, 1)}
    if x.dx0 is not None:
        out["dx"] = x.dx0 + stack(dxs, 1)
    return out


# ======================================================================================================= shade_in / sigmoid
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _shade_norm(x):
    g = [x.g[:, k] for k in range(3)]
    J = [[x.jinv[:, 3 * k + j] for j in range(3)] for k in range(3)]
    v = [g[0] * J[0][j] + g[1] * J[1][j] + g[2] * J[2][j] for j in range(3)]
    na = _dot3(v, v).sqrt()
    a = na.clamp_min(1e-12)
    n1 = [vj / a for vj in v]
    nb = _dot3(n1, n1).sqrt()
    b = nb.clamp_min(1e-6)
    return g, J, v, na, a, n1, nb, b, [q / b for q in n1]


def tree_shade_in_fwd(x):
    return {"nrm": stack(_shade_norm(x)[-1], 1)}


def r_shade_normal(g, jinv):
    v = (g.unsqueeze(1) @ jinv.view(-1, 3, 3)).squeeze(1)
    return F.normalize(F.normalize(v, dim=-1, eps=1e-12), dim=-1, eps=1e-6)


def ref_shade_in_fwd(x):
    return {"nrm": r_shade_normal(x.g, x.jinv)}


def _dn(x):
    return x.dXR[:, 3:6] + x.dnrm_extra if x.dnrm_extra is not None else x.dXR[:, 3:6]


def ref_shade_in_bwd(x):
    g, J = _leaf(x.g), _leaf(x.jinv)
    loss = (r_shade_normal(g, J) * _dn(x)).sum()
    return {"dg": _grad(loss, g, True).detach(), "djinv": _grad(loss, J, False).detach()}


def tree_shade_in_bwd(x):
    g, J, v, na, a, n1, nb, b, n = _shade_norm(x)
    dn = [x.dXR[:, 3 + j] + (x.dnrm_extra[:, j] if x.dnrm_extra is not None else 0.0) for j in range(3)]
    dot = _dot3(dn, n)
    m = gt(nb, 1e-6)
    dn1 = [where(m, (dn[j] - n[j] * dot) / b, dn[j] / b) for j in range(3)]
    dot = _dot3(dn1, n1)
    m = gt(na, 1e-12)
    dv = [where(m, (dn1[j] - n1[j] * dot) / a, dn1[j] / a) for j in range(3)]
    dg = [dv[0] * J[k][0] + dv[1] * J[k][1] + dv[2] * J[k][2] for k in range(3)]
    return {"dg": stack(dg, 1), "djinv": stack([g[k] * dv[j] for k in range(3) for j in range(3)], 1)}


def ref_sigmoid_fwd(x):
    return {"Y": 1.0 / (1.0 + torch.exp(-x.Z))}


def tree_sigmoid_fwd(x):
    return {"Y": 1.0 / (1.0 + (-x.Z).exp())}


def ref_sigmoid_bwd(x):
    return {"dZ": x.dY * x.Y * (1.0 - x.Y)}


def tree_sigmoid_bwd(x):
    return {"dZ": x.dY * x.Y * (1.0 - x.Y)}


# ============================================================================================================ weight norm
def r_wn(v, g):
    return v if g is None else v * (g / v.norm(dim=1)).unsqueeze(1)


def ref_wn_fwd(x):
    return {"W": r_wn(x.v, x.g)}


def tree_wn_fwd(x):
    if x.g is None:
        return {"W": x.v * 1.0}
    s = x.g / tsum(x.v * x.v, 1).sqrt()
    return {"W": x.v * s.unsqueeze(1)}


def ref_wn_bwd(x):
    if x.g is None:
        return {"dv": x.dW.clone()}
    v, g = _leaf(x.v), _leaf(x.g)
    loss = (r_wn(v, g) * x.dW).sum()
    return {"dv": _grad(loss, v, True).detach(), "dg": _grad(loss, g, False).detach()}


def tree_wn_bwd(x):
    if x.g is None:
        return {"dv": x.dW * 1.0}
    ss, dot = tsum(x.v * x.v, 1), tsum(x.dW * x.v, 1)
    nrm = ss.sqrt()
    return {"dv": (x.g / nrm).unsqueeze(1) * (x.dW - (dot / ss).unsqueeze(1) * x.v), "dg": dot / nrm}


def wn_layout(shapes, with_g, order_seed):
    """descriptors of a multi-layer launch: -> (row0 of every layer, total rows, dW / dv / dg float offsets in SHUFFLED,
    non-contiguous order (7 floats of slack between the blocks), sizes of the acc and grad buffers)"""
    row0, r = [], 0
    for o, i in shapes:
        row0.append(r)
        r += o
    perm = torch.randperm(len(shapes), generator=torch.Generator().manual_seed(order_seed)).tolist()
    dW_off, dv_off, dg_off = [0] * len(shapes), [0] * len(shapes), [0] * len(shapes)
    a = gpos = 5
    for li in perm:
        o, i = shapes[li]
        dW_off[li] = a
        a += o * i + 7
    for li in reversed(perm):
        o, i = shapes[li]
        dv_off[li] = gpos
        gpos += o * i + 7
        if with_g[li]:
            dg_off[li] = gpos
            gpos += o + 7
    return row0, r, dW_off, dv_off, dg_off, a, gpos


def wn_find(row0, row):
    """the kernels' descriptor lookup: the last layer whose first row is <= row"""
    lo, hi = 0, len(row0) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if row0[mid] <= row:
            lo = mid
        else:
            hi = mid - 1
    return lo, row - row0[lo]


def ref_wn_fwd_multi(layers, row0, total_rows):
    """the multi-layer forward as the kernel sees it: one block per row of the concatenated range -> list of W"""
    out = [torch.zeros_like(v, dtype=torch.float64) for v, _ in layers]
    for row in range(total_rows):
        li, r = wn_find(row0, row)
        v, g = layers[li]
        if r < v.shape[0]:
            out[li][r] = r_wn(v[r:r + 1].double(), None if g is None else g[r:r + 1].double())[0]
    return out


# ================================================================================================= hoist / colsum / copies
def ref_hoist_fwd(x):
    return {"b2": x.b + x.W[:, x.c0:x.c0 + x.n] @ x.vec}


def tree_hoist_fwd(x):
    return {"b2": x.b + tsum(x.W[:, x.c0:x.c0 + x.n] * x.vec.unsqueeze(0), 1)}


def ref_hoist_bwd(x):
    dW = x.dW0.clone()
    dW[:, x.c0:x.c0 + x.n] += x.db2.unsqueeze(1) * x.vec.unsqueeze(0)
    return {"dW": dW}


def ref_colsum(x, drop_last=False):
    return {"db": x.dZ[:x.rows - (1 if drop_last else 0)].sum(0)}


def tree_colsum(x):
    return {"db": tsum(x.dZ[:x.rows], 0)}


def copy_cols_candidates(src, scale, dst0, accumulate):
    """float32 results that mp_tr_copy_cols may return: fl(s x) | fl(fl(s x) + d) or fl(s x + d) (a contracted fma)"""
    p64 = src.double() * scale
    if not accumulate:
        return [p64.float()]
    return [(p64.float().double() + dst0.double()).float(), (p64 + dst0.double()).float()]


# ============================================================================================================== bg_comp
def r_bg_comp(sdf, rgb, zbg):
    dist = torch.cat([zbg[:, :-1] - zbg[:, 1:], torch.full_like(zbg[:, :1], 1e10)], 1)
    fe = dist * sdf.abs()
    front = torch.cat([torch.zeros_like(fe[:, :1]), torch.cumsum(fe, 1)[:, :-1]], 1)
    w = (1.0 - torch.exp(-fe)) * torch.exp(-front)
    return (w.unsqueeze(-1) * rgb).sum(1)


def ref_bg_comp_fwd(x):
    return {"out": r_bg_comp(x.sdf, x.rgb, x.zbg)}


def ref_bg_comp_bwd(x):
    s, c = _leaf(x.sdf), _leaf(x.rgb)
    loss = (r_bg_comp(s, c, x.zbg) * x.dout).sum()
    return {"dsdf": _grad(loss, s, True).detach(), "drgb": _grad(loss, c, False).detach()}


def _bg_dist(x, i, NBG):
    return x.zbg[:, i] - x.zbg[:, i + 1] if i + 1 < NBG else full(x.zbg[:, i], 1e10)


def tree_bg_comp_fwd(x):
    NBG = x.sdf.shape[1]
    csum = full(x.sdf[:, 0], 0.0)
    acc = [full(x.sdf[:, 0], 0.0) for _ in range(3)]
    for i in range(NBG):
        fe = _bg_dist(x, i, NBG) * x.sdf[:, i].abs()
        w = (1.0 - (-fe).exp()) * (-csum).exp()
        acc = [acc[a] + w * x.rgb[:, i, a] for a in range(3)]
        csum = csum + fe
    return {"out": stack(acc, 1)}


def tree_bg_comp_bwd(x):
    NBG = x.sdf.shape[1]
    E = full(x.sdf[:, 0], 0.0)
    for i in range(NBG - 1):
        E = E + _bg_dist(x, i, NBG) * x.sdf[:, i].abs()
    suffix = full(x.sdf[:, 0], 0.0)
    dsdf, drgb = [None] * NBG, [None] * NBG
    raw = x.sdf.v if isinstance(x.sdf, EB) else x.sdf
    for i in range(NBG - 1, -1, -1):
        dist = _bg_dist(x, i, NBG)
        fe = dist * x.sdf[:, i].abs()
        if i + 1 < NBG:
            E = E - fe
        T, ex = (-E).exp(), (-fe).exp()
        w = (1.0 - ex) * T
        dw = x.dout[:, 0] * x.rgb[:, i, 0] + x.dout[:, 1] * x.rgb[:, i, 1] + x.dout[:, 2] * x.rgb[:, i, 2]
        dfe = dw * T * ex - suffix
        sgn = torch.sign(raw[:, i])
        dsdf[i] = dfe * dist * (EB(sgn.double()) if isinstance(x.sdf, EB) else sgn)
        drgb[i] = stack([w * x.dout[:, a] for a in range(3)], 1)
        suffix = suffix + dw * w
    return {"dsdf": stack(dsdf, 1), "drgb": stack(drgb, 1)}


# ============================================================================================================== warp_bwd
def r_warp(tfs, x_posed, w, wc):
    """x_c = (sum_j w_j T_j)^-1 [x; 1] and Jinv = (sum_j wc_j T_j[:3,:3])^-1, float64"""
    Tm = torch.einsum("ij,jab->iab", w, tfs)
    xc = torch.linalg.solve(Tm[:, :3, :3], (x_posed - Tm[:, :3, 3]).unsqueeze(-1)).squeeze(-1)
    jinv = torch.linalg.inv(torch.einsum("ij,jab->iab", wc, tfs[:, :3, :3]))
    return xc, jinv


def ref_warp_bwd(x):
    T = _leaf(x.tfs.view(NJ, 4, 4))
    xc, jinv = r_warp(T, x.x_posed, x.skin_w[x.nn_posed], x.skin_w[x.nn_cano])
    loss = (xc * x.dxc).sum()
    if x.djinv is not None:
        loss = loss + (jinv.reshape(-1, 9) * x.djinv).sum()
    return {"dtfs": (x.dtfs0.view(NJ, 4, 4) + _grad(loss, T, False)).detach().view(NJ, 16)}


def tree_warp_bwd(x):
    w = take(x.skin_w, x.nn_posed)                                            # [n][24]
    tl = x.tfs
    R = [tsum(w * tl[:, 4 * a + b].unsqueeze(0), 1) for a in range(3) for b in range(3)]
    c0, c1, c2 = R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6]
    r = 1.0 / (R[0] * c0 + R[1] * c1 + R[2] * c2)
    I = [c0 * r, (R[2] * R[7] - R[1] * R[8]) * r, (R[1] * R[5] - R[2] * R[4]) * r,
         c1 * r, (R[0] * R[8] - R[2] * R[6]) * r, (R[2] * R[3] - R[0] * R[5]) * r,
         c2 * r, (R[1] * R[6] - R[0] * R[7]) * r, (R[0] * R[4] - R[1] * R[3]) * r]
    d = [x.dxc[:, a] for a in range(3)]
    q = [with_input_rounding(x.xc[:, a]) for a in range(3)]
    u = [I[a] * d[0] + I[3 + a] * d[1] + I[6 + a] * d[2] for a in range(3)]
    dT = {}
    for a in range(3):
        for b in range(3):
            dT[4 * a + b] = -u[a] * q[b]
        dT[4 * a + 3] = -u[a]
    tot = {e: tsum(w * dT[e].unsqueeze(1), 0) for e in dT}                     # [24] per entry
    if x.djinv is not None:
        M = [with_input_rounding(x.jinv[:, k]) for k in range(9)]
        dM = [x.djinv[:, k] for k in range(9)]
        t1 = [M[a] * dM[b] + M[3 + a] * dM[3 + b] + M[6 + a] * dM[6 + b] for a in range(3) for b in range(3)]
        wc = take(x.skin_w, x.nn_cano)
        for a in range(3):
            for b in range(3):
                dRc = -(t1[3 * a] * M[3 * b] + t1[3 * a + 1] * M[3 * b + 1] + t1[3 * a + 2] * M[3 * b + 2])
                tot[4 * a + b] = tot[4 * a + b] + tsum(wc * dRc.unsqueeze(1), 0)
    cols = [x.dtfs0[:, e] + tot[e] if e in tot else x.dtfs0[:, e] * 1.0 for e in range(16)]
    return {"dtfs": stack(cols, 1)}


def ref_gather_bwd(x):
    verts = torch.zeros(x.n_verts, 3, dtype=torch.float64, requires_grad=True)
    if x.idx.numel() == 0:
        return {"dverts": x.dverts0.clone()}
    xc = (x.jinv.view(-1, 3, 3) @ verts[x.idx].unsqueeze(-1)).squeeze(-1)
    return {"dverts": (x.dverts0 + _grad((xc * x.dxc).sum(), verts, False)).detach()}


# ================================================================================================================ registry
REFS = {"softplus_fwd": ref_softplus_fwd, "softplus_bwd": ref_softplus_bwd, "sigmul": ref_sigmul, "rev_adj": ref_rev_adj,
        "dz": ref_dz, "rev_chain": ref_rev_chain, "pe": ref_pe, "pe_bwd": ref_pe_bwd, "pe_grad_fwd": ref_pe_grad_fwd,
        "pe_grad_bwd": ref_pe_grad_bwd, "shade_in_fwd": ref_shade_in_fwd, "shade_in_bwd": ref_shade_in_bwd,
        "sigmoid_fwd": ref_sigmoid_fwd, "sigmoid_bwd": ref_sigmoid_bwd, "wn_fwd": ref_wn_fwd, "wn_bwd": ref_wn_bwd,
        "hoist_fwd": ref_hoist_fwd, "colsum": ref_colsum, "bg_comp_fwd": ref_bg_comp_fwd, "bg_comp_bwd": ref_bg_comp_bwd,
        "warp_bwd": ref_warp_bwd}
TREES = {"softplus_fwd": tree_softplus_fwd, "softplus_bwd": tree_softplus_bwd, "sigmul": tree_sigmul, "rev_adj": tree_rev_adj,
         "dz": tree_dz, "rev_chain": tree_rev_chain, "pe": tree_pe, "pe_bwd": tree_pe_bwd, "pe_grad_fwd": tree_pe_grad_fwd,
         "pe_grad_bwd": tree_pe_grad_bwd, "shade_in_fwd": tree_shade_in_fwd, "shade_in_bwd": tree_shade_in_bwd,
         "sigmoid_fwd": tree_sigmoid_fwd, "sigmoid_bwd": tree_sigmoid_bwd, "wn_fwd": tree_wn_fwd, "wn_bwd": tree_wn_bwd,
         "hoist_fwd": tree_hoist_fwd, "colsum": tree_colsum, "bg_comp_fwd": tree_bg_comp_fwd, "bg_comp_bwd": tree_bg_comp_bwd,
         "warp_bwd": tree_warp_bwd}
BOUNDED = tuple(TREES)


def _conv(inp, f):
    d = {}
    for k, v in inp.items():
        d[k] = f(v) if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v
    if "Z" in inp:
        d["hi"] = softplus_hi(inp["Z"])
    return NS(**d)


def reference(name, inp, **kw):
    """float64 reference outputs of kernel `name` on the float32 inputs `inp`"""
    return REFS[name](_conv(inp, lambda t: t.double()), **kw)


def bounds(name, inp):
    """per-element error bounds (float64) of every output"""
    return {k: o.e + FLOOR for k, o in TREES[name](_conv(inp, EB.lift)).items()}


def emulate(name, inp):
    """the kernel's expression tree in the host's float32"""
    return TREES[name](_conv(inp, lambda t: t))


def worst_ratio(got, want64, bound):
    """max |got - want| / bound over the elements; NaN or inf anywhere in got counts as inf"""
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    if g.numel() == 0:
        return 0.0
    return float(((g - want64).abs() / bound).max())


def ratios(name, inp, got=None):
    """{output: worst ratio}; got None: the float32 emulation"""
    ref, bnd = reference(name, inp), bounds(name, inp)
    got = emulate(name, inp) if got is None else got
    return {k: worst_ratio(got[k], ref[k], bnd[k].expand_as(ref[k])) for k in bnd}


# ============================================================================================================ input cases
def _g(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return (scale * torch.randn(*shape, generator=_g(seed), dtype=torch.float64)).float()


def ints(shape, seed, max_abs=8):
    return torch.randint(-max_abs, max_abs + 1, tuple(shape), generator=_g(seed), dtype=torch.int64).float()


def case_softplus(rows, C, P, seed, scale=1.0):
    Z = softplus_z(P if P > 0 else rows, C, seed)
    if P > 0:
        Z = torch.cat([Z, randn((3 * P, C), seed + 1, 0.5)], 0)
    return {"Z": Z, "P": P, "scale": f32(scale), "dH": randn((Z.shape[0], C), seed + 2)}


def case_rev(rows, C, seed, use_U=True):
    d = {"Z": softplus_z(rows, C, seed), "U": randn((rows, C), seed + 1) if use_U else None, "wrow": randn((C,), seed + 2),
         "scale": f32(1 / math.sqrt(2)), "uscale": f32(1 / math.sqrt(2)), "dV": randn((rows, C), seed + 3),
         "dX": randn((rows, C), seed + 4), "dS": randn((rows, C), seed + 5)}
    return d


def pe_points(P, D, seed):
    x = (3.0 * torch.rand(P, D, generator=_g(seed), dtype=torch.float64) - 1.5).float()
    x.view(-1)[:3] = torch.tensor([0.0, 1.0, -1.0])[:min(3, x.numel())]
    return x


def case_pe(P, D, L, fwd, scale, seed):
    rows = 4 * P if fwd else P
    return {"x": pe_points(P, D, seed), "L": L, "fwd": fwd, "scale": f32(scale), "dIN": randn((rows, pe_width(D, L)), seed + 1),
            "dx0": randn((P, D), seed + 2)}


def case_pe_grad(P, L, seed, with_dx=True):
    return {"x": pe_points(P, 3, seed), "L": L, "G": randn((P, pe_width(3, L)), seed + 1), "dgrad": randn((P, 3), seed + 2),
            "dx0": randn((P, 3), seed + 3) if with_dx else None}


def case_shade(n, seed, extra=True):
    """point 0: zero gradient (both clamps active); point 1: a Jinv far from orthonormal"""
    g = randn((n, 3), seed)
    g[0] = 0.0
    jinv = (torch.eye(3).view(1, 9) + randn((n, 9), seed + 1, 0.2)).contiguous()
    if n > 1:
        jinv[1] = torch.tensor([3.0, 2.5, 0.0, 0.0, 0.05, 1.0, -2.0, 0.0, 0.3])
    return {"g": g, "jinv": jinv, "dXR": randn((n, 6), seed + 2), "dnrm_extra": randn((n, 3), seed + 3) if extra else None,
            "xc": randn((n, 3), seed + 4), "dsdf": randn((n,), seed + 5), "sdf": randn((n,), seed + 6)}


def case_wn(out_dim, in_dim, seed, with_g=True):
    return {"v": randn((out_dim, in_dim), seed, 0.3), "g": (randn((out_dim,), seed + 1).abs() + 0.5) if with_g else None,
            "dW": randn((out_dim, in_dim), seed + 2)}


def case_bg(R, NBG, seed):
    sdf = randn((R, NBG), seed, 0.3)
    sdf.view(-1)[::5] = 0.0                                        # exact zeros, the first sample among them
    if NBG > 1:
        sdf[0, -1] = 0.0                                           # and a last sample (the 1e10 interval)
    zbg = torch.sort(0.05 + 0.9 * torch.rand(R, NBG, generator=_g(seed + 1), dtype=torch.float64), 1, descending=True)[0].float()
    return {"sdf": sdf, "rgb": torch.rand(R, NBG, 3, generator=_g(seed + 2)), "zbg": zbg, "dout": randn((R, 3), seed + 3)}


def rigid(n, seed):
    """n rigid motions times a scale in [0.8, 1.2], float32 [n][16]"""
    g = _g(seed)
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.linalg.det(q)).view(n, 1, 1)
    T = torch.zeros(n, 4, 4, dtype=torch.float64)
    T[:, :3, :3] = q * (0.8 + 0.4 * torch.rand(n, 1, 1, generator=g, dtype=torch.float64))
    T[:, :3, 3] = 0.3 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    T[:, 3, 3] = 1.0
    return T.float().view(n, 16)


def case_warp(n, seed, with_djinv=True, n_verts=40):
    g = _g(seed)
    skin = torch.zeros(n_verts, NJ, dtype=torch.float64)
    for v in range(n_verts):                                       # 4-sparse rows; vertex 0 one-hot
        js = torch.randperm(NJ, generator=g)[:1 if v == 0 else 4]
        wv = torch.rand(len(js), generator=g, dtype=torch.float64) + 0.1
        skin[v, js] = wv / wv.sum()
    skin = skin.float()
    tfs = rigid(NJ, seed + 1)
    nn_posed = torch.randint(0, n_verts, (n,), generator=g)
    nn_cano = torch.randint(0, n_verts, (n,), generator=g)
    nn_posed[0] = 0
    x_posed = torch.randn(n, 3, generator=g, dtype=torch.float64)
    xc, jinv = r_warp(tfs.double().view(NJ, 4, 4), x_posed, skin.double()[nn_posed], skin.double()[nn_cano])
    return {"xc": xc.float(), "jinv": jinv.reshape(n, 9).float().contiguous(), "x_posed": x_posed, "dxc": randn((n, 3), seed + 2),
            "djinv": randn((n, 9), seed + 3) if with_djinv else None, "nn_posed": nn_posed, "nn_cano": nn_cano,
            "skin_w": skin, "tfs": tfs, "dtfs0": randn((NJ, 16), seed + 4)}


# the cases the CPU ratios of tests/tolerances_train_elementwise.py are measured on (deterministic, a fraction of a second)
def cpu_ratio_cases():
    c = {}
    c["softplus_fwd"] = [case_softplus(64, 8, 0, 1), case_softplus(20, 8, 5, 2, 1 / math.sqrt(2))]
    c["softplus_bwd"] = [case_softplus(64, 8, 0, 3), case_softplus(20, 8, 5, 4, 1 / math.sqrt(2))]
    for k in ("sigmul", "rev_adj", "dz", "rev_chain"):
        c[k] = [case_rev(64, 8, 5), case_rev(64, 8, 6, use_U=False)]
    c["pe"] = [case_pe(64, 3, 10, 1, 1.0, 7), case_pe(64, 4, 6, 0, 1 / math.sqrt(2), 8)]
    c["pe_bwd"] = c["pe"]
    c["pe_grad_fwd"] = c["pe_grad_bwd"] = [case_pe_grad(64, 6, 9), case_pe_grad(64, 10, 10)]
    c["shade_in_fwd"] = c["shade_in_bwd"] = [case_shade(300, 11), case_shade(5, 12, extra=False)]
    c["sigmoid_fwd"] = [{"Z": randn((1000,), 13, 3.0)}]
    c["sigmoid_bwd"] = [{"Y": torch.rand(1000, generator=_g(14)), "dY": randn((1000,), 15)}]
    c["wn_fwd"] = c["wn_bwd"] = [case_wn(8, 65, 16), case_wn(5, 270, 17), case_wn(3, 39, 18)]
    c["hoist_fwd"] = [{"W": randn((8, 90), 19), "b": randn((8,), 20), "c0": 14, "n": 69, "vec": randn((69,), 21)}]
    c["colsum"] = [{"dZ": randn((1000, 3), 22), "rows": 1000}, {"dZ": randn((257, 8), 23), "rows": 255}]
    c["bg_comp_fwd"] = c["bg_comp_bwd"] = [case_bg(64, 33, 24), case_bg(64, 2, 25), case_bg(9, 1, 26)]
    c["warp_bwd"] = [case_warp(700, 27), case_warp(257, 28, with_djinv=False)]
    return c


def cpu_ratios():
    """{kernel: worst ratio of the host's float32 tree to the bound (U_F = 1) over cpu_ratio_cases()}"""
    out = {}
    for name, cases in cpu_ratio_cases().items():
        out[name] = max(max(ratios(name, inp).values()) for inp in cases)
    return out
