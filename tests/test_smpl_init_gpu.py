"""The mesh fit on the device (csrc/fit.hip, multiply_amd/smpl_init.py): each kernel against the float64 restatement of
tests/test_smpl_init_cpu.py, one step's gradients and the whole fit against a plain torch statement, the body-shaped result and
the render with the warm start.  Bounds: tests/tolerances_smpl_init.py."""

import numpy as np
import pytest
import torch

from oracle import multiply_oracle as O
from tests import tolerances_smpl_init as TS
from tests.test_smpl_init_cpu import icosphere, ref_area_cdf, ref_loss, ref_sample
from tests.util import seeded_networks, t32

pytestmark = pytest.mark.gpu


def rel(name, got, want):
    got, want = got.double().cpu(), want.double().cpu()
    e = (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)
    print(f"[smpl_init] {name}: rel-to-max err {e:.3e} (|want|max {want.abs().max().item():.3e})")
    return e


def rel_l2(name, got, want):
    got, want = got.double().cpu().reshape(-1), want.double().cpu().reshape(-1)
    e = ((got - want).norm() / (want.norm() + 1e-30)).item()
    print(f"[smpl_init] {name}: relative L2 {e:.3e} (|want| {want.norm().item():.3e})")
    return e


def unequal_mesh(seed=0, n=500):
    """triangles whose areas span six decades, with degenerate faces (a repeated vertex) first, in the middle and last"""
    g = torch.Generator().manual_seed(seed)
    size = 10.0 ** (torch.rand(n, generator=g) * 3.0 - 3.0)
    c = (torch.rand(n, 1, 3, generator=g) - 0.5)
    fv = c + (torch.rand(n, 3, 3, generator=g) - 0.5) * size[:, None, None]
    for k in (0, n // 2, n // 2 + 1, n - 1):
        fv[k, 1] = fv[k, 0]
    # coordinates on a 2^-12 lattice: the edge vectors are then exact in fp32, so the kernel's normals of the SMALL faces can
    # meet the 1e-6 bound at all (an fp32 difference of two coordinates ~0.5 apart by 1e-3 carries only 1e-4 relative accuracy)
    return (torch.round(fv * 4096.0) / 4096.0).contiguous()


# ------------------------------------------------------------------------------------------------ 1. sampling
@pytest.mark.parametrize("mesh", ["icosphere", "unequal"])
def test_area_cdf_and_sample_against_restatement(mesh):
    from multiply_amd import hip
    if mesh == "icosphere":
        v, f = icosphere(3)
        fv = v[f].contiguous()
    else:
        fv = unequal_mesh()
    area, normal, cdf = hip.fit_area_cdf(fv.cuda())
    w_area, w_normal, w_cdf = ref_area_cdf(fv)
    assert rel("area", area, w_area) < 1e-6 and (normal.cpu().double() - w_normal).abs().max() < TS.SAMPLE_POINT
    assert (cdf.cpu().double() - w_cdf).abs().max() < 2e-7 and cdf[-1].item() == 1.0
    assert ((area == 0).cpu() == (w_area == 0)).all()
    g = torch.Generator().manual_seed(1)
    n_s, n_near, n_box = 20001, 7001, 3000                               # ragged against the 256-point workgroups
    u_surf, z, u_box = torch.rand(n_s, 3, generator=g), torch.randn(n_near, 3, generator=g), torch.rand(n_box, 3, generator=g)
    box = torch.tensor([[-0.7, -0.8, -0.9], [0.9, 0.8, 0.7]])
    pts, nrm, fid = hip.fit_sample(fv.cuda(), normal, cdf, u_surf.cuda(), z.cuda(), 0.05, u_box.cuda(), box.cuda())
    torch.cuda.synchronize()
    w_pts, w_nrm, w_fid, w_vol = ref_sample(fv, w_normal, w_cdf, u_surf, z, 0.05, u_box, box)
    fid = fid.cpu().long()
    differ = fid != w_fid
    near_step = ((u_surf[:, :1].double() - w_cdf[None]).abs() < TS.SAMPLE_CDF_EPS).any(1)
    print(f"[smpl_init] {mesh}: {int(differ.sum())} of {n_s} face ids differ, {int(near_step.sum())} uniforms within 1e-6 of a CDF step")
    assert not (differ & ~near_step).any() and differ.sum() <= TS.SAMPLE_EXCUSED * n_s
    assert (w_area[fid] > 0).all(), "a degenerate face was selected"
    same = ~differ
    e_p = (pts[:n_s].cpu().double() - w_pts).abs()[same].max().item()
    e_n = (nrm.cpu().double() - w_nrm).abs()[same].max().item()
    near_same = same[torch.arange(n_near) % n_s]
    e_v = torch.cat([(pts[n_s:n_s + n_near].cpu().double() - w_vol[:n_near]).abs()[near_same].reshape(-1),
                     (pts[n_s + n_near:].cpu().double() - w_vol[n_near:]).abs().reshape(-1)]).max().item()
    print(f"[smpl_init] {mesh}: surface points {e_p:.2e}, normals {e_n:.2e}, volume points {e_v:.2e}")
    assert max(e_p, e_n, e_v) < TS.SAMPLE_POINT
    # the near-surface volume points are copies of the device's own surface points plus the offset (one fused multiply-add apart)
    k = torch.arange(n_near, device="cuda") % n_s
    assert (pts[n_s:n_s + n_near] - (pts[:n_s][k] + 0.05 * z.cuda())).abs().max() < 2e-7


@pytest.mark.parametrize("mesh", ["icosphere", "unequal"])
def test_face_selection_follows_the_areas(mesh):
    from scipy.stats import chi2
    from multiply_amd import hip
    fv = unequal_mesh() if mesh == "unequal" else (lambda v, f: v[f].contiguous())(*icosphere(2))
    area, normal, cdf = hip.fit_area_cdf(fv.cuda())
    n = 1_000_000
    g = torch.Generator(device="cuda").manual_seed(7)
    u = torch.rand(n, 3, generator=g, device="cuda")
    _, _, fid = hip.fit_sample(fv.cuda(), normal, cdf, u, torch.zeros(0, 3, device="cuda"), 0.0, torch.zeros(0, 3, device="cuda"),
                               torch.zeros(2, 3, device="cuda"))
    counts = torch.bincount(fid.long(), minlength=fv.shape[0]).cpu().double()
    w_area = ref_area_cdf(fv)[0]
    assert (counts[w_area == 0] == 0).all()
    # pool the faces expected fewer than 5 times (the chi-square approximation needs cells that are not tiny)
    exp = n * w_area / w_area.sum()
    big = exp >= 5
    obs_c = torch.cat([counts[big], counts[~big].sum()[None]])
    exp_c = torch.cat([exp[big], exp[~big].sum()[None]])
    keep = exp_c > 0
    stat = float((((obs_c - exp_c) ** 2)[keep] / exp_c[keep]).sum())
    crit = float(chi2.isf(TS.CHI2_LEVEL, int(keep.sum()) - 1))
    print(f"[smpl_init] {mesh}: chi-square {stat:.1f} over {int(keep.sum())} cells, critical value at 1e-4: {crit:.1f}")
    assert stat < crit


# ------------------------------------------------------------------------------------------------ 2. loss
def _loss_inputs(n_s, n_v, seed, special=True):
    g = torch.Generator().manual_seed(seed)
    n = n_s + n_v
    sdf = torch.randn(n, generator=g) * 0.3
    grad = torch.randn(n, 3, generator=g)
    grad = grad / grad.norm(dim=1, keepdim=True) * (1.0 + 0.3 * torch.randn(n, 1, generator=g))
    normals = torch.randn(n_s, 3, generator=g)
    normals = normals / normals.norm(dim=1, keepdim=True)
    dist = torch.randn(n_v, generator=g) * 0.3
    if special and n >= 63:                     # the special branches: zero-norm gradient, gradient == normal, sdf == 0, sdf == dist
        grad[0] = 0.0
        sdf[1] = 0.0
        if n_s > 3:
            grad[2] = normals[2]
        if n_v > 2:
            sdf[n_s + 1] = dist[1]
            grad[n_s] = 0.0
    return sdf, grad, normals, dist


@pytest.mark.parametrize("n_s,n_v", [(1, 0), (0, 1), (1, 1), (63, 0), (31, 32), (64, 1), (65, 64), (8192, 8192), (0, 65), (1000, 37)])
@pytest.mark.parametrize("tau", [0.0, 0.25])
def test_fit_loss_against_float64_autograd(n_s, n_v, tau):
    from multiply_amd import hip
    sdf, grad, normals, dist = _loss_inputs(n_s, n_v, seed=n_s + 3 * n_v)
    w = (1.0, 0.7, 1.3, 0.1)
    s64, g64 = sdf.double().requires_grad_(True), grad.double().requires_grad_(True)
    want = ref_loss(s64, g64, normals.double(), dist.double(), w, tau)
    want[0].backward()
    dev = [t.cuda() for t in (sdf, grad, normals, dist)]
    terms, d_sdf, d_grad = hip.fit_loss(*dev, w, tau)
    terms2, d_sdf2, d_grad2 = hip.fit_loss(*dev, w, tau)
    torch.cuda.synchronize()
    assert torch.equal(terms, terms2) and torch.equal(d_sdf, d_sdf2) and torch.equal(d_grad, d_grad2), "two calls differ"
    assert torch.isfinite(terms).all() and torch.isfinite(d_grad).all()
    for k, name in enumerate(("total", "surface", "normal", "distance", "eikonal")):
        e = abs(terms[k].item() - want[k].item()) / max(abs(want[k].item()), 1e-30) if want[k].item() != 0 else abs(terms[k].item())
        print(f"[smpl_init] loss {n_s}+{n_v} tau {tau}: {name} {terms[k].item():.6e} want {want[k].item():.6e} rel {e:.2e}")
        assert e < TS.LOSS_REL, name
    assert rel("d_sdf", d_sdf, s64.grad) < TS.LOSS_REL
    assert rel("d_grad", d_grad, g64.grad) < TS.LOSS_REL


# ------------------------------------------------------------------------------------------------ 3. one step's gradients
def _net(seed=0, perturb=False):
    m, _ = seeded_networks(1, seed)
    net = m.foreground_implicit_network_list[0].cuda()
    if perturb:                                 # as tests/test_train_gpu.py::test_fused_sdf_kernels_against_autograd
        torch.manual_seed(11)
        with torch.no_grad():
            for prm in net.parameters():
                prm.add_(torch.randn_like(prm) * 0.02 * prm.abs().mean().clamp_min(1e-2))
    return net


def _torch_loss(net, pts, nrm, dist, cond, cfg):
    """network + objective as plain torch (fp32, autograd with create_graph) on given points"""
    sd = dict(net.named_parameters())
    x = pts.detach().clone().requires_grad_(True)
    out = O.implicit_forward(sd, "", x, cond, 6)
    g = torch.autograd.grad(out[:, 0].sum(), x, create_graph=True)[0]
    return ref_loss(out[:, 0], g, nrm, dist, cfg.weights, cfg.truncation)


def test_one_fit_step_gradients_against_autograd():
    from multiply_amd import hip
    from multiply_amd import smpl_init as S
    from multiply_amd import train as T
    net = _net(perturb=True)
    v, f = icosphere(3)
    cfg = S.FitConfig(n_surface=1500, n_volume=1300, seed=3)
    target = S.MeshTarget(v, f, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(3)
    pts, nrm, fid, dist = S.fit_step_points(target, cfg, S.fit_box(cfg, target.verts, "cuda"), S.make_draws(cfg, gen, "cuda"))
    cond = torch.zeros(69, device="cuda")
    ev = T.ImplicitTrainFused(net, pts, cond)
    terms, d_sdf, d_grad = hip.fit_loss(ev.sdf, ev.grad, nrm, dist, cfg.weights, cfg.truncation)
    ev.backward(torch.zeros(pts.shape[0], 256, device="cuda"), d_sdf, d_grad)
    got = dict(zip([id(p) for p in ev.params()], ev.param_grads()))
    want_terms = _torch_loss(net, pts, nrm, dist, cond, cfg)
    names, plist = zip(*net.named_parameters())
    want = torch.autograd.grad(want_terms[0], plist, allow_unused=True)
    e = abs(terms[0].item() - want_terms[0].item()) / abs(want_terms[0].item())
    print(f"[smpl_init] one step: loss {terms[0].item():.6e} vs torch {want_terms[0].item():.6e}, rel {e:.2e}")
    assert e < TS.STEP_LOSS_REL
    assert len(got) == len(plist)
    for n, p, ww in zip(names, plist, want):
        assert rel_l2(n, got[id(p)].reshape(p.shape), ww) < TS.PARAM_GRAD_REL_L2, n


# ------------------------------------------------------------------------------------------------ 4. the fit vs a torch fit
FIT4 = dict(n_surface=2048, n_volume=2048, steps=200)


def torch_fit(net, v, f, cfg):
    """the whole loop as plain torch: the fit's draws (same seeded device generator), the float64 sampling map, the float64
    exact distance (the oracle's), network + objective under autograd in fp32, torch's Adam.  Returns the loss of every step."""
    fv = v[f]
    area, normal, cdf = ref_area_cdf(fv)
    from multiply_amd import smpl_init as S
    box = S.fit_box(cfg, v.cuda(), "cuda").cpu()
    gen = torch.Generator(device="cuda").manual_seed(cfg.seed)
    cond = torch.zeros(69, device="cuda")
    opt = torch.optim.Adam(list(net.parameters()), lr=cfg.lr)
    losses = []
    for _ in range(cfg.steps):
        u_surf, z, u_box = [t.cpu() for t in S.make_draws(cfg, gen, "cuda")]
        pts, nrm, _, vol = ref_sample(fv, normal, cdf, u_surf, z, cfg.sigma_local, u_box, box)
        dist = O.mesh_signed_distance(vol, fv)
        terms = _torch_loss(net, torch.cat([pts, vol]).float().cuda(), nrm.float().cuda(), dist.float().cuda(), cond, cfg)
        opt.zero_grad(set_to_none=True)
        terms[0].backward()
        opt.step()
        losses.append(float(terms[0]))
    return losses


def heldout_mean(net, v, f):
    from multiply_amd import smpl_init as S
    h = S.heldout_error(net, v, f, n_surface=4096, n_box=4096)
    return 0.5 * (h["surface_mean"] + h["box_mean"])


def fit_pair(seed, device_fit=True):
    """(error before, device fit's error and step-1 loss, torch fit's error and step-1 loss) for one seed"""
    from multiply_amd import smpl_init as S
    v, f = icosphere(2)
    cfg = S.FitConfig(seed=seed, **FIT4)
    before = heldout_mean(_net(), v, f)
    dev_err = dev_l1 = None
    if device_fit:
        net_d = _net()
        rec = S.fit_implicit_net(net_d, v, f, cfg=cfg, log_every=cfg.steps)
        dev_err, dev_l1 = heldout_mean(net_d, v, f), rec.terms[0][1]["total"]
    net_t = _net()
    losses = torch_fit(net_t, v, f, cfg)
    return before, dev_err, dev_l1, heldout_mean(net_t, v, f), losses[0]


def test_fit_converges_like_a_torch_fit():
    """Measured on MI355X (profiles/smpl_init_fit.txt): see tests/tolerances_smpl_init.py FIT_RATIO_MAX / FIT_GAIN_MIN."""
    before, dev_err, dev_l1, ref_err, ref_l1 = fit_pair(0)
    e1 = abs(dev_l1 - ref_l1) / abs(ref_l1)
    ratio, gain_dev, gain_ref = dev_err / ref_err, before / dev_err, before / ref_err
    print(f"[smpl_init] fit vs torch fit: step-1 loss {dev_l1:.6e} vs {ref_l1:.6e} (rel {e1:.2e}); held-out mean |sdf - d| before "
          f"{before:.4e}, device fit {dev_err:.4e}, torch fit {ref_err:.4e}: ratio {ratio:.3f}, gain {gain_dev:.2f} vs {gain_ref:.2f}")
    assert e1 < TS.STEP_LOSS_REL
    assert ratio < TS.FIT_RATIO_MAX
    assert gain_dev > TS.FIT_GAIN_MIN


# ------------------------------------------------------------------------------------------------ 5. / 6. the body-shaped result
def _scene(P=2, H=32, W=32, smpl_init_path=None):
    import warnings
    warnings.filterwarnings("ignore")
    from multiply_amd.config import load_config
    from multiply_amd.multiply import Multiply
    from multiply_amd.synthetic import make_scene, make_smpl_tables
    tables = make_smpl_tables(0)
    sc = make_scene(P, seed=0, H=H, W=W)
    opt = load_config()
    if smpl_init_path is not None:
        opt.smpl_init = True
        opt.smpl_init_path = smpl_init_path
    torch.manual_seed(0)
    model = Multiply(opt, sc["smpl_params"][0, :, 76:], smpl_tables=tables).eval()
    sp = t32(sc["smpl_params"])
    inp = dict(uv=t32(sc["uv"]), intrinsics=t32(sc["intrinsics"]), pose=t32(sc["pose"]), smpl_params=sp,
               smpl_pose=sp[:, :, 4:76], smpl_shape=sp[:, :, 76:], smpl_trans=sp[:, :, 1:4], idx=torch.tensor([3]))
    return model, inp, tables, sc


@pytest.fixture(scope="module")
def body_fit(tmp_path_factory):
    """person 0 of the synthetic scene fitted to closed_body_mesh with the DEFAULT config, saved with save_smpl_init"""
    from multiply_amd import smpl_init as S
    from multiply_amd.synthetic import closed_body_mesh
    model, _, _, _ = _scene()
    with pytest.raises(ValueError, match="exactly two faces"):        # the tables' own `f` is not a surface
        S.fit_smpl_init(model, str(tmp_path_factory.mktemp("refused") / "x.pth"), person=0)
    v, f = closed_body_mesh(model.smpl_server_list[0])
    assert S.mesh_is_closed(f)
    path = str(tmp_path_factory.mktemp("smpl_init") / "smpl_init_synthetic.pth")
    net, rec = S.fit_smpl_init(model, path, person=0, mesh=(v, f), log_every=500)
    print(f"[smpl_init] body: {v.shape[0]} vertices, {f.shape[0]} faces; {rec}")
    return dict(model=model, net=net, rec=rec, path=path, v=v, f=f)


def test_body_fit_quality_and_file(body_fit):
    from multiply_amd import hip
    from multiply_amd import mesh as M
    from multiply_amd import smpl_init as S
    net, v, f = body_fit["net"], body_fit["v"], body_fit["f"]
    h = S.heldout_error(net, v, f)
    ex = M.canonical_mesh(body_fit["model"], 0)
    d = hip.mesh_signed_distance(ex.vertices_t.float().contiguous(), v[f].contiguous()).abs()
    h["levelset_mean"], h["levelset_max"] = float(d.mean()), float(d.max())
    print("[smpl_init] body fit: " + ", ".join(f"{k} {x:.4e}" for k, x in h.items()) + f"; level set {ex.faces.shape[0]} faces")
    for k, x in h.items():
        assert x < TS.BODY[k], k
    model2, _, _, _ = _scene(smpl_init_path=body_fit["path"])
    want = net.state_dict()
    for imp in model2.foreground_implicit_network_list:
        got = imp.state_dict()
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k


def _max_preactivation(net, x, cond):
    sd = {k: p.detach() for k, p in net.named_parameters()}
    emb = O.fourier_embed(x, 6)
    h, zmax = emb, 0.0
    for l in range(9):
        w, b = O.linear_params(sd, "", l)
        if l == 0:
            h = torch.cat([h, cond.view(1, -1).expand(h.shape[0], -1)], -1)
        if l == 4:
            h = torch.cat([h, emb], 1) / np.sqrt(2)
        h = torch.nn.functional.linear(h, w, b)
        if l < 8:
            zmax = max(zmax, float(h.abs().max()))
            h = O.softplus100(h)
    return zmax


def test_render_with_the_warm_start_against_oracle(body_fit):
    from multiply_amd import hip
    from tests.test_render_gpu import report
    model, inp, tables, sc = _scene(smpl_init_path=body_fit["path"])
    got = model({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()})
    torch.cuda.synchronize()
    n_hit = model.last_stats["n_hit"]
    hit = [model._last["per"][p]["hit_index"][:n].long().cpu() for p, n in zip(model._last["persons"], n_hit)]
    print("[smpl_init] warm-start render: hit rays per person", n_hit, "of", inp["uv"].shape[1])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want = O.MultiplyOracle(sd, tables, sc["smpl_params"][0, :, 76:]).forward_eval(inp, hit)
    for k in ("rgb_values", "fg_rgb_values", "acc_map", "acc_person_list", "normal_values"):
        st = report("warm start " + k, got[k], want[k])
        assert st[0] < TS.RENDER[k][0] and st[1] < TS.RENDER[k][1], k
    # the fitted networks stay inside the f16 kernels' range: scaled pre-activations |z'| = K |z| < 454
    x = (torch.rand(20000, 3, device="cuda") - 0.5) * 2.4
    pose = inp["smpl_pose"][0, :, 3:].cuda()
    for p, imp in enumerate(model.foreground_implicit_network_list):
        z = max(_max_preactivation(imp, x, torch.zeros(69, device="cuda")), _max_preactivation(imp, x, pose[p]))
        print(f"[smpl_init] person {p}: largest scaled pre-activation {z * hip.SOFTPLUS_K:.1f} (limit {TS.F16_PREACT})")
        assert z * hip.SOFTPLUS_K < TS.F16_PREACT
