"""Deterministic weight regimes for the inference network kernels, and their float64 reference.

The parity tests of tests/test_mlp_gpu.py run on the seeded geometric init only: the SDF net is close to a sphere, nearly
every softplus unit is saturated, and the colour nets output close to a constant.  The regimes here exercise what the
half-precision kernels are built to survive (csrc/mlp_core.hpp):

  geometric   tests.util.seeded_networks as it stands (the control).
  trained     every ImplicitNet layer: weight_v (plain `weight` for the background net) perturbed by Gaussian noise of 0.4x its
              RMS, biases drawn at the scale of the weights' contribution, and a per-layer gain on weight_g chosen on a seeded
              calibration set so that the pre-activations z of the hidden layers have an RMS of 0.15 -- a clear fraction of the
              beta = 100 softplus units is then in transition (|100 z| < 5); make_regime asserts >= 10 % per hidden layer on the
              test points.  The last layer's sdf bias is shifted so that the sdf has median 0 over the canonical region (the
              zero set crosses it).  The rendering nets (foreground and background) are redrawn with nn.Linear's default init
              (weight_v = the drawn weight, weight_g = its row norms) and non-zero biases, then given per-layer gains so that
              every layer's pre-activations have unit RMS and the output pre-sigmoid an RMS of 1.5 around zero mean:
              make_regime asserts a per-channel std of the rgb >= 0.1.  Feature vectors are what these implicit nets produce.
  near_range  `trained`, with the first hidden layer of the foreground SDF nets (weight_g and bias of lin0) scaled by one
              factor s, chosen by bisection on the float64 reference so that the largest pre-activation over the canonical region
              is NEAR_RANGE_FRACTION of the f16 limit below (softplus is positively homogeneous for large arguments: every later
              layer grows with s as well).
  beyond_range the same at BEYOND_RANGE_FRACTION of the limit (the overflow contract test).

The f16 limit, derived from csrc/mlp_core.hpp.  The softplus networks run in SCALED UNITS: the host multiplies the biases and
input-fed weights by K = 100 log2(e) = 144.27 (hip.py implicit_plans), so a hidden layer's fp32 accumulator holds z' = K z.  Its
rows are rounded to half precision by ONE v_cvt_pk_f16_f32 (to_h2, round to nearest even) before the activation; the largest
finite half is 65504, and an accumulator of 65520 or more becomes +-inf.  The activation h' = max(z', 0) + log2(1 + 2^-|z'|)
is then <= max(z', 0) + 1 and is stored as a half as well.  Hence |z| < Z_LIMIT = 65504 / K = 454.0 in the network's own units
(the skip layer's inputs are divided by sqrt(2) on the host, in the same units as the reference's, so the same bound holds for
every hidden layer).  The forward-mode kernel carries the tangent columns d z' / dx at K * TANGENT_SCALE = 9.0 per unit:
|dz/dx| < TANGENT_LIMIT = 65504 / 9.0 = 7278 -- measured by max_preactivation as well, it binds later than the values here.
"""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from oracle import multiply_oracle as O

REGIMES = ("geometric", "trained", "near_range")
K = 100.0 * math.log2(math.e)                      # scaled units of the softplus networks (hip.SOFTPLUS_K)
F16_MAX = 65504.0
TANGENT_SCALE = 0.0625                             # mlp_core.hpp: forward-mode tangent columns carried at 1/16
Z_LIMIT = F16_MAX / K                              # 454.0: largest |pre-activation| the half-precision kernels represent
TANGENT_LIMIT = F16_MAX / (K * TANGENT_SCALE)      # 7278: largest |d z / d x| of the forward-mode kernel
NEAR_RANGE_FRACTION = 0.7
BEYOND_RANGE_FRACTION = 1.2
TRANSITION = 5.0                                   # a softplus unit is in transition where |100 z| < 5
MIN_TRANSITION_FRACTION = 0.10
MIN_RGB_STD = 0.10
FG_PREFIX = "foreground_implicit_network_list.0."
FG_REN_PREFIX = "foreground_rendering_network_list.0."
BG_PREFIX = "bg_implicit_network."
BG_REN_PREFIX = "bg_rendering_network."
FRAME = 7                                          # the background's frame code: row of frame_latent_encoder.weight


# ------------------------------------------------------------------------------------------------ test inputs
def canonical_bounds(margin=0.2):
    """box of the canonical ("A-pose") body of the synthetic SMPL tables the suite uses, plus `margin` on every side: the
    points the deformer can return lie within max_dist of the body"""
    from multiply_amd.synthetic import make_smpl_tables
    srv = O.SMPLServerOracle(O.SMPLTables(make_smpl_tables(0)), np.zeros(10, np.float32))
    v = srv.verts_c.reshape(-1, 3).double()
    return v.min(0).values - margin, v.max(0).values + margin


def region_points(n, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)
    return lo + (hi - lo) * torch.rand(n, 3, generator=g, dtype=torch.float64)


def pose_vector(seed):
    """body pose conditioning (69,) at the scale of real poses (0.3 rad per axis), not N(0, 0.1)"""
    return 0.3 * torch.randn(69, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def bg_rays(n, seed):
    """(dirs, cam) of one camera near the centre of the scene sphere: a third of the rays along +-x / +-y / +-z (the
    inverse-sphere points then have a coordinate at +-1: the 10-octave Fourier features see their largest arguments, 2^9 rad),
    the rest random directions; every ray carries the 32 inverse depths of bg_depths (the 4th coordinate spans [0, 1/r])"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    ax = torch.cat([torch.eye(3, dtype=torch.float64), -torch.eye(3, dtype=torch.float64)])
    k = torch.arange(n) % 3 == 0
    d[k] = ax[torch.arange(int(k.sum())) % 6] + 1e-3 * torch.randn(int(k.sum()), 3, generator=g, dtype=torch.float64)
    return F.normalize(d, dim=1), torch.tensor([0.03, -0.02, 0.01], dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ float64 reference
def to64(sd, device="cpu"):
    return {k: v.detach().to(device=device, dtype=torch.float64) for k, v in sd.items()}


def implicit_preacts(sd, prefix, x, cond, multires, tangents=False, skip_in=(4,), n_lin=9):
    """the oracle's ImplicitNet formulas (O.implicit_forward) with the pre-activation of every hidden layer returned:
    (out, [z_0 .. z_7]) and, with `tangents`, [d z_l / d x] (N, width, 3) for the forward-mode range"""
    emb = O.fourier_embed(x, multires)
    h, zs, ts = emb, [], []
    if tangents:
        eye = torch.eye(x.shape[1], dtype=x.dtype, device=x.device)
        temb = torch.func.vmap(lambda v: torch.func.jvp(lambda y: O.fourier_embed(y, multires), (x,), (v.expand_as(x),))[1])(eye)
        temb = temb.permute(1, 2, 0)                                     # (N, E, 3)
        th = temb
    for l in range(n_lin):
        w, b = O.linear_params(sd, prefix, l)
        if l == 0 and cond is not None:
            h = torch.cat([h, cond.view(1, -1).expand(h.shape[0], -1)], -1)
            if tangents:
                th = torch.cat([th, th.new_zeros(th.shape[0], cond.numel(), th.shape[2])], 1)
        if l in skip_in:
            h = torch.cat([h, emb], 1) / np.sqrt(2)
            if tangents:
                th = torch.cat([th, temb], 1) / np.sqrt(2)
        h = F.linear(h, w, b)
        if tangents:
            th = torch.einsum("oi,nic->noc", w, th)
        if l < n_lin - 1:
            zs.append(h)
            if tangents:
                ts.append(th)
                th = th * torch.sigmoid(100.0 * h)[..., None]
            h = O.softplus100(h)
    return h, zs, ts


def transition_fraction(zs):
    return [float(((100.0 * z).abs() < TRANSITION).double().mean()) for z in zs]


def max_preactivation(zs):
    return max(float(z.abs().max()) for z in zs)


def fg_reference(sd, x, cond, jinv, with_normals=True):
    """sdf, features, normals (autograd through the oracle's formulas, then Jinv as in multiply.py:606-661) and rgb of
    person 0 at canonical points; every tensor in the dtype / on the device of `sd`"""
    xg = x.detach().clone().requires_grad_(with_normals)
    out = O.implicit_forward(sd, FG_PREFIX, xg, cond, multires=6)
    if with_normals:
        g = torch.autograd.grad(out[:, :1], xg, torch.ones_like(out[:, :1]))[0]
        nrm = F.normalize(F.normalize(torch.einsum("bi,bij->bj", g, jinv), dim=1), dim=-1, eps=1e-6)
    else:
        g, nrm = None, F.normalize(torch.ones_like(x), dim=1)
    out = out.detach()
    rgb = O.rendering_forward_pose_no_view(sd, FG_REN_PREFIX, x, nrm, cond, out[:, 1:])
    return dict(sdf=out[:, 0], feat=out[:, 1:], grad=g, nrm=nrm, rgb=rgb)


def bg_reference(sd, dirs, cam, radius=3.0, n_bg=32, chunk=512):
    """MultiplyOracle.background (multiply.py:514-539, 682-726) in the dtype / on the device of `sd`"""
    frame_code = sd["frame_latent_encoder.weight"][FRAME]
    cfg = O.SamplerCfg(radius=radius, N_bg=n_bg)
    outs = []
    for s in range(0, dirs.shape[0], chunk):
        d = dirs[s:s + chunk]
        R = d.shape[0]
        c = cam.reshape(1, 3).expand(R, -1)
        z_bg = torch.flip(O.bg_depths(cfg, R), dims=[-1]).to(d)
        pts = O.depth2pts_outside(c[:, None, :].expand(-1, n_bg, -1), d[:, None, :].expand(-1, n_bg, -1), z_bg,
                                  radius).reshape(-1, 4)
        out = O.implicit_forward(sd, BG_PREFIX, pts, frame_code, multires=10)
        rgb = O.rendering_forward_nerf_frame(sd, BG_REN_PREFIX, d[:, None, :].expand(-1, n_bg, -1).reshape(-1, 3), out[:, 1:],
                                             frame_code)
        dens = out[:, :1].abs().reshape(-1, n_bg)
        dists = torch.cat([z_bg[:, :-1] - z_bg[:, 1:], 1e10 * torch.ones_like(z_bg[:, :1])], -1)
        free = dists * dens
        shifted = torch.cat([torch.zeros_like(free[:, :1]), free[:, :-1]], -1)
        w = (1 - torch.exp(-free)) * torch.exp(-torch.cumsum(shifted, -1))           # O.bg_volume_weights, in the input dtype
        outs.append((w[:, :, None] * rgb.reshape(-1, n_bg, 3)).sum(1))
    return torch.cat(outs)


def bg_points(dirs, cam, radius=3.0, n_bg=32):
    cam = cam.reshape(1, 3).expand(dirs.shape[0], -1)
    z_bg = torch.flip(O.bg_depths(O.SamplerCfg(radius=radius, N_bg=n_bg), dirs.shape[0]), dims=[-1]).to(dirs)
    return O.depth2pts_outside(cam[:, None, :].expand(-1, n_bg, -1), dirs[:, None, :].expand(-1, n_bg, -1), z_bg,
                               radius).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ weight regimes
def _wv(lin):
    return lin.weight_v if hasattr(lin, "weight_v") else lin.weight


def _scale_rows(lin, c):
    """multiply the effective weight of `lin` by c (per row or scalar): weight_g for weight-normed layers"""
    if hasattr(lin, "weight_g"):
        lin.weight_g.mul_(torch.as_tensor(c, dtype=lin.weight_g.dtype).reshape(-1, 1) if torch.is_tensor(c) else c)
    else:
        lin.weight.mul_(torch.as_tensor(c, dtype=lin.weight.dtype).reshape(-1, 1) if torch.is_tensor(c) else c)


def _eff64(lin):
    from multiply_amd.networks import effective_weight
    return effective_weight(lin).detach().double()


def _train_implicit(net, x, cond, multires, g, z_rms=0.15, bias_rms=0.5):
    """perturb + calibrate an ImplicitNet in place, layer by layer on the calibration inputs x (float64)"""
    emb = O.fourier_embed(x, multires)
    h = emb
    lins = net.layers()
    for l, lin in enumerate(lins):
        v = _wv(lin)
        v.add_(0.4 * v.pow(2).mean().sqrt() * torch.randn(v.shape, generator=g))
        if l == 0 and cond is not None:
            h = torch.cat([h, cond.view(1, -1).expand(h.shape[0], -1)], -1)
        if l in net.skip_in:
            h = torch.cat([h, emb], 1) / np.sqrt(2)
        if l == len(lins) - 1:
            # sdf row keeps its (perturbed) geometric scale; feature rows get biases like the hidden layers; the sdf bias is
            # shifted so that the sdf has median 0 on the calibration points (the zero set crosses the region)
            lin.bias[1:] = 0.1 * torch.randn(lin.bias.shape[0] - 1, generator=g)
            z = F.linear(h, _eff64(lin), lin.bias.detach().double())
            lin.bias[0] -= float(z[:, 0].median())
            break
        wz = F.linear(h, _eff64(lin))
        c = z_rms * (1.0 - bias_rms ** 2) ** 0.5 / float(wz.pow(2).mean().sqrt())   # bias_rms: the biases' share
        _scale_rows(lin, c)
        lin.bias.copy_(bias_rms * z_rms * torch.randn(lin.bias.shape, generator=g))
        h = O.softplus100(F.linear(h, _eff64(lin), lin.bias.detach().double()))


def _redraw_rendering(net, inputs, g, out_rms=1.5):
    """nn.Linear default init (kaiming-uniform weights, uniform non-zero biases), then per-layer gains: hidden
    pre-activations of unit RMS, output pre-sigmoid of RMS out_rms per channel around zero mean"""
    h = inputs
    lins = net.layers()
    for l, lin in enumerate(lins):
        n_out, n_in = _wv(lin).shape
        bound = 1.0 / math.sqrt(n_in)
        w = (torch.rand(n_out, n_in, generator=g) * 2 - 1) * bound                   # = kaiming_uniform_(a=sqrt(5))
        b = (torch.rand(n_out, generator=g) * 2 - 1) * bound
        if hasattr(lin, "weight_g"):
            lin.weight_v.copy_(w)
            lin.weight_g.copy_(w.norm(dim=1, keepdim=True))
        else:
            lin.weight.copy_(w)
        lin.bias.copy_(b)
        z = F.linear(h, _eff64(lin), lin.bias.detach().double())
        if l < len(lins) - 1:
            c = 1.0 / float(z.pow(2).mean().sqrt())
            _scale_rows(lin, c)
            lin.bias.mul_(c)
            h = torch.relu(z * c)
        else:
            zc = z - z.mean(0)
            c = out_rms / zc.pow(2).mean(0).sqrt()                                    # per output channel
            _scale_rows(lin, c.float())
            lin.bias.copy_((c * (lin.bias.detach().double() - z.mean(0))).float())


def _fg_scale(m, factor, x=None, cond=None):
    """lin0 of the foreground SDF nets x factor; with calibration points x, the sdf bias is re-centred (median 0 on x)"""
    for p, net in enumerate(m.foreground_implicit_network_list):
        lin = net.layers()[0]
        _scale_rows(lin, factor)
        lin.bias.mul_(factor)
        if x is not None:
            sdf = O.implicit_forward(to64(m.state_dict(), x.device), f"foreground_implicit_network_list.{p}.", x, cond, multires=6)[:, 0]
            net.layers()[-1].bias[0] -= float(sdf.median())


def _max_pre_fg(m, x, cond):
    sd = to64(m.state_dict(), x.device)
    return max(max_preactivation(implicit_preacts(sd, f"foreground_implicit_network_list.{p}.", x, cond, 6)[1])
               for p in range(len(m.foreground_implicit_network_list)))


def regime_networks(regime, seed=0, device="cpu"):
    """(module, opt, info): the seeded scene networks (tests.util.seeded_networks(2, seed)) turned into `regime`; float32
    parameters on the CPU; info = what the regime was calibrated to (`scale`, `max_pre` for the range regimes)"""
    from tests.util import seeded_networks
    warnings.filterwarnings("ignore")
    m, opt = seeded_networks(2, seed)
    info = {}
    if regime == "geometric":
        return m, opt, info
    g = torch.Generator().manual_seed(1000 + seed)
    lo, hi = canonical_bounds()
    xc = region_points(1024, 2000 + seed, lo, hi)
    cond = pose_vector(3000 + seed)
    with torch.no_grad():
        for p, (imp, ren) in enumerate(zip(m.foreground_implicit_network_list, m.foreground_rendering_network_list)):
            _train_implicit(imp, xc, cond, 6, g)
            sd = to64(m.state_dict())
            out = O.implicit_forward(sd, f"foreground_implicit_network_list.{p}.", xc, cond, multires=6)
            ren.lin_pose.weight.copy_((torch.rand(ren.lin_pose.weight.shape, generator=g) * 2 - 1) / math.sqrt(69))
            ren.lin_pose.bias.copy_((torch.rand(8, generator=g) * 2 - 1) / math.sqrt(69))
            pose8 = F.linear(cond.view(1, -1), ren.lin_pose.weight.double(), ren.lin_pose.bias.double())
            nrm = F.normalize(torch.randn(xc.shape, generator=g, dtype=torch.float64), dim=1)
            _redraw_rendering(ren, torch.cat([xc, nrm, pose8.expand(xc.shape[0], -1), out[:, 1:]], 1), g)
        d, c = bg_rays(128, 4000 + seed)
        code = m.frame_latent_encoder.weight[FRAME].detach().double()
        pts = bg_points(d, c)
        _train_implicit(m.bg_implicit_network, pts, code, 10, g)
        out = O.implicit_forward(to64(m.state_dict()), BG_PREFIX, pts, code, multires=10)
        vd = d[:, None, :].expand(-1, 32, -1).reshape(-1, 3)
        _redraw_rendering(m.bg_rendering_network,
                          torch.cat([O.fourier_embed(vd, 4), code.view(1, -1).expand(vd.shape[0], -1), out[:, 1:]], 1), g)
        if regime in ("near_range", "beyond_range"):
            target = (NEAR_RANGE_FRACTION if regime == "near_range" else BEYOND_RANGE_FRACTION) * Z_LIMIT
            xs = region_points(2048, 5000 + seed, lo, hi).to(device)
            cond_d = cond.to(device)
            base = _max_pre_fg(m, xs, cond_d)
            # bisection on log s: the largest pre-activation grows monotonically (and nearly linearly) with the scale of lin0
            a, b = 0.0, math.log(4 * target / base)
            ref = {k: v.clone() for k, v in m.state_dict().items()}
            for _ in range(30):
                mid = 0.5 * (a + b)
                m.load_state_dict(ref)
                _fg_scale(m, math.exp(mid))
                if _max_pre_fg(m, xs, cond_d) < target:
                    a = mid
                else:
                    b = mid
                if b - a < 2e-3:
                    break
            m.load_state_dict(ref)
            _fg_scale(m, math.exp(a), xc, cond)
            info.update(scale=math.exp(a), max_pre=_max_pre_fg(m, xs, cond_d))
    return m, opt, info


def surface_points(sd, prefix, cond, lo, hi, n, seed, iters=48):
    """n points on the float64 zero set of the sdf inside [lo, hi]: bisection on segments between random points of opposite
    sign"""
    dev = lo.device
    g = torch.Generator().manual_seed(seed)
    found = []
    for _ in range(20):
        if sum(len(f) for f in found) >= n:
            break
        a = region_points(4 * n, int(torch.randint(1 << 30, (1,), generator=g)), lo.cpu(), hi.cpu()).to(dev)
        b = region_points(4 * n, int(torch.randint(1 << 30, (1,), generator=g)), lo.cpu(), hi.cpu()).to(dev)
        fa = O.implicit_forward(sd, prefix, a, cond, multires=6)[:, 0]
        fb = O.implicit_forward(sd, prefix, b, cond, multires=6)[:, 0]
        k = (fa * fb) < 0
        a, b, fa = a[k], b[k], fa[k]
        for _ in range(iters):
            mid = 0.5 * (a + b)
            fm = O.implicit_forward(sd, prefix, mid, cond, multires=6)[:, 0]
            same = (fm * fa) > 0
            a = torch.where(same[:, None], mid, a)
            fa = torch.where(same, fm, fa)
            b = torch.where(same[:, None], b, mid)
        found.append(0.5 * (a + b))
    assert sum(len(f) for f in found) >= n, "the sdf has (almost) no zero set in the region"
    return torch.cat(found)[:n]


class Regime:
    """networks of one regime + the float64 reference on its test inputs.

    fg: person 0's ImplicitNet / RenderingNet at N_FG canonical points (region points over the canonical bounds and points on the
    float64 zero set, interleaved so that every prefix holds both), pose conditioning, per-point Jinv; bg: N_BG rays of
    bg_rays.  The regime's promises are asserted here: a regime that turns out degenerate fails loudly."""

    def __init__(self, regime, n_fg=4099, n_bg=4099, seed=0, device="cpu", normals=True):
        self.name = regime
        self.m, self.opt, self.info = regime_networks(regime, seed, device)
        self.device = device
        self.sd32 = {k: v.detach().clone() for k, v in self.m.state_dict().items()}
        self.sd = to64(self.sd32, device)
        lo, hi = canonical_bounds()
        n_surf = n_fg // 3
        xr = region_points(n_fg - n_surf, 6000 + seed, lo, hi).to(device)
        self.cond = pose_vector(7000 + seed).to(device)
        xs = surface_points(self.sd, FG_PREFIX, self.cond, lo.to(device), hi.to(device), n_surf, 8000 + seed)
        x = torch.cat([xr, xs])
        order = torch.randperm(n_fg, generator=torch.Generator().manual_seed(9000 + seed))
        self.on_surface = (order >= xr.shape[0]).to(device)
        self.x = x[order.to(device)]
        g = torch.Generator().manual_seed(9100 + seed)
        A = 0.3 * torch.randn(n_fg, 3, 3, generator=g, dtype=torch.float64) + torch.eye(3, dtype=torch.float64)
        self.jinv = torch.linalg.inv(A).to(device)
        self.fg = fg_reference(self.sd, self.x, self.cond, self.jinv, with_normals=normals)
        _, zs, ts = implicit_preacts(self.sd, FG_PREFIX, self.x, self.cond, 6, tangents=normals)
        self.frac_transition = transition_fraction(zs)
        self.point_max_pre = torch.stack([z.abs().max(1).values for z in zs]).max(0).values   # per point, over the hidden layers
        self.max_pre = max_preactivation(zs)
        self.max_tangent = max(float(t.abs().max()) for t in ts) if ts else None
        self.dirs, self.cam = (t.to(device) for t in bg_rays(n_bg, 9200 + seed))
        self.bg_rgb = bg_reference(self.sd, self.dirs, self.cam)
        _, zb, _ = implicit_preacts(self.sd, BG_PREFIX, bg_points(self.dirs[:256], self.cam),
                                    self.sd["frame_latent_encoder.weight"][FRAME], 10)
        self.bg_frac_transition = transition_fraction(zb)
        self.fg_rgb_std = [float(s) for s in self.fg["rgb"].std(0)]
        self.bg_rgb_std = [float(s) for s in self.bg_rgb.std(0)]
        if regime == "trained":
            assert min(self.frac_transition) >= MIN_TRANSITION_FRACTION, f"fg units in transition per layer: {self.frac_transition}"
            assert min(self.bg_frac_transition) >= MIN_TRANSITION_FRACTION, \
                f"bg units in transition per layer: {self.bg_frac_transition}"
            assert min(self.fg_rgb_std) >= MIN_RGB_STD, f"fg rgb std per channel: {self.fg_rgb_std}"
            assert min(self.bg_rgb_std) >= MIN_RGB_STD, f"bg rgb std per channel: {self.bg_rgb_std}"
        if regime in ("near_range", "beyond_range"):
            frac = NEAR_RANGE_FRACTION if regime == "near_range" else BEYOND_RANGE_FRACTION
            assert 0.9 * frac <= self.max_pre / Z_LIMIT <= 1.1 * frac, (self.max_pre / Z_LIMIT, frac)

    def summary(self):
        t = "" if self.max_tangent is None else f", max |dz/dx| {self.max_tangent:.1f} ({self.max_tangent / TANGENT_LIMIT:.3f} of the limit)"
        return (f"regime {self.name}: fg units in transition per layer {[round(f, 3) for f in self.frac_transition]}, "
                f"bg {[round(f, 3) for f in self.bg_frac_transition]}; max |z| {self.max_pre:.2f} ({self.max_pre / Z_LIMIT:.3f} of "
                f"the f16 limit){t}; rgb std fg {[round(s, 3) for s in self.fg_rgb_std]} bg {[round(s, 3) for s in self.bg_rgb_std]}; "
                f"{self.info}")
