"""The feature fold (hip.FoldedColor, mp_fold_features, mp_mlp_shade_rev_fold, mp_background_fold) against the unfolded entry
points and the float64 reference of tests/weight_regimes.py.

Only the shade -> colour hand-off changes: the SDF network stops at its sdf row and hands on its last hidden vector, the colour
network's first layer carries the product of the two linear layers.  So sdf and normals are torch.equal between the two paths,
and the colours of both are held to the bounds the unfolded path already has (tests/tolerances.py MLP_BY_REGIME, TOL.EVAL): no
tolerance of its own.  Point counts 1, 255, 256, 257, 513: a lone point, a tile boundary of the 256-point tiles and ragged last
tiles.  The geometric regime has the largest share of folded weights below the smallest normal half (6.1e-5): it is the one that
would show a matrix unit that flushes subnormal operands."""
import pytest
import torch

from tests import tolerances as TOL
from tests import weight_regimes as W

pytestmark = pytest.mark.gpu

COUNTS = (1, 255, 256, 257, 513)
BG_RAYS = (1, 2, 3, 300)
WG = 256                      # persistent grid (csrc/mlp.hip grid_for)
N_WRAP = 2 * 65536 + 77       # every workgroup runs at least two 256-point tiles
_CACHE = {}


def regime(name):
    if name not in _CACHE:
        R = W.Regime(name, n_fg=max(COUNTS), n_bg=max(BG_RAYS), device="cuda")
        R.m.cuda()
        _CACHE[name] = R
    return _CACHE[name]


def max_abs(got, want):
    return float((got.double() - want.double()).abs().max())


def check(tag, value, bound):
    print(f"[fold] {tag}: {value:.3e} (bound {bound:.1e})")
    return value < bound


def chunks(n, step):
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def test_fold_kernel_against_float64():
    """mp_fold_features: the product, the bias and the untouched columns against float64, foreground and background pair"""
    from multiply_amd import hip
    from multiply_amd.networks import effective_weight
    for name in W.REGIMES:
        m = regime(name).m
        for ren, imp, ks_in in ((m.foreground_rendering_network_list[0], m.foreground_implicit_network_list[0], 2),
                                (m.bg_rendering_network, m.bg_implicit_network, 3)):
            fc = hip.folded_color(ren, imp, ks_in)
            fc.refresh(None)
            torch.cuda.synchronize()
            wc, w8 = effective_weight(fc.lin_c).detach().double(), effective_weight(fc.lin_8).detach().double()
            c0 = fc.col0
            want = wc.clone()
            want[:, c0:] = wc[:, c0:] @ w8[1:]
            want_b = fc.lin_c.bias.detach().double() + wc[:, c0:] @ fc.lin_8.bias.detach().double()[1:]
            # fp32: a serial sum of 256 fused products (<= 256 u of the sum of magnitudes, u = 2^-24) of factors that each carry
            # the few roundings of the weight norm (<= 8 u together)
            mag = wc[:, c0:].abs() @ w8[1:].abs()
            bound = (256 + 8) * 2.0 ** -24 * float(mag.max())
            e_w, e_b = max_abs(fc.folded.weight, want), max_abs(fc.folded.bias, want_b)
            mag_b = fc.lin_c.bias.detach().double().abs() + wc[:, c0:].abs() @ fc.lin_8.bias.detach().double()[1:].abs()
            bound_b = (256 + 8) * 2.0 ** -24 * float(mag_b.max())
            print(f"[fold] {name} ks_in={ks_in} folded weight max|err| {e_w:.3e} (bound {bound:.1e}), bias {e_b:.3e} (bound {bound_b:.1e})")
            assert e_w <= bound and e_b <= bound_b
            # the other columns: the effective weight itself (fp32 weight norm: a few ulp)
            assert max_abs(fc.folded.weight[:, :c0], wc[:, :c0]) <= 2.0 ** -21 * float(wc.abs().max())


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", W.REGIMES)
def test_foreground(name, n):
    """(sdf, normal, rgb) through the folded and the unfolded reverse-mode entry points on the same points"""
    from multiply_amd import hip
    R, tol = regime(name), TOL.MLP_BY_REGIME[name]
    imp, ren = R.m.foreground_implicit_network_list[0], R.m.foreground_rendering_network_list[0]
    x, jinv, cond = R.x[:n].float(), R.jinv[:n].float(), R.cond.float()
    plain = hip.shade_points(imp, ren, x, jinv, cond, mode="reverse")
    fold = hip.shade_points(imp, ren, x, jinv, cond, mode="reverse", fold=True)
    torch.cuda.synchronize()
    assert torch.equal(plain[0], fold[0]), "sdf"
    assert torch.equal(plain[1], fold[1]), "normal"
    ok = [check(f"{name} n={n} shade rgb (unfolded) max|err|", max_abs(plain[2], R.fg["rgb"][:n]), tol["shade_rgb"]),
          check(f"{name} n={n} shade rgb (folded) max|err|", max_abs(fold[2], R.fg["rgb"][:n]), tol["shade_rgb"])]
    print(f"[fold] {name} n={n} rgb folded vs unfolded max|diff| {max_abs(fold[2], plain[2]):.3e}")
    assert all(ok)


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("name", W.REGIMES)
def test_folded_color_on_reference_inputs(name, n):
    """mp_mlp_color with the folded pack on the float64 points, normals and last hidden vector of the regime's implicit net (what
    test_rendering_net of tests/test_mlp_weights_gpu.py does with the features): the colour network's own bound"""
    import ctypes as C
    from multiply_amd import hip
    from oracle import multiply_oracle as O
    R, tol = regime(name), TOL.MLP_BY_REGIME[name]
    imp, ren = R.m.foreground_implicit_network_list[0], R.m.foreground_rendering_network_list[0]
    if "h7" not in R.__dict__:
        R.h7 = O.softplus100(W.implicit_preacts(R.sd, W.FG_PREFIX, R.x, R.cond, 6)[1][-1])
    x, nrm, cond = R.x[:n].float().contiguous(), R.fg["nrm"][:n].float().contiguous(), R.cond.float().contiguous()
    frag = hip.pack_feature_fragments((hip.SOFTPLUS_K * R.h7[:n]).float())
    pk = hip.folded_color(ren, imp, 2).refresh(hip.pose_embed(ren)(cond))
    rgb = torch.empty(n, 3, device="cuda")
    hip.lib().mp_mlp_color(C.byref(pk.net), pk.wpack, pk.bias, x, nrm, frag, None, None, n, rgb, hip.stream())
    got_plain = ren(x, nrm, None, cond[None], R.fg["feat"][:n].float())
    torch.cuda.synchronize()
    ok = [check(f"{name} n={n} colour rgb (unfolded) max|err|", max_abs(got_plain, R.fg["rgb"][:n]), tol["color_rgb"]),
          check(f"{name} n={n} colour rgb (folded) max|err|", max_abs(rgb, R.fg["rgb"][:n]), tol["color_rgb"])]
    assert all(ok)


@pytest.mark.parametrize("n", BG_RAYS)
@pytest.mark.parametrize("name", W.REGIMES)
def test_background(name, n):
    from multiply_amd import hip
    from oracle import multiply_oracle as O
    R, tol = regime(name), TOL.MLP_BY_REGIME[name]
    m = R.m
    z = torch.flip(O.bg_depths(O.SamplerCfg(), 1), dims=[-1])[0].cuda()
    code = m.frame_latent_encoder.weight[W.FRAME].detach()
    run = lambda fold: hip.background(m.bg_implicit_network, m.bg_rendering_network, R.dirs[:n].float(), R.cam.float(), z, code,
                                      fold=fold)
    plain, fold = run(False), run(True)
    torch.cuda.synchronize()
    ok = [check(f"{name} rays={n} background rgb (unfolded) max|err|", max_abs(plain, R.bg_rgb[:n]), tol["bg_rgb"]),
          check(f"{name} rays={n} background rgb (folded) max|err|", max_abs(fold, R.bg_rgb[:n]), tol["bg_rgb"])]
    assert all(ok)


# ---------------------------------------------------------------------------------------------------------------- ring wrap
def wrap_scene():
    if "wrap" not in _CACHE:
        m = regime("trained").m
        lo, hi = W.canonical_bounds()
        g = torch.Generator().manual_seed(78)
        _CACHE["wrap"] = dict(m=m, x=W.region_points(N_WRAP, 7003, lo, hi).float().cuda().contiguous(),
                              cond=W.pose_vector(3000).float().cuda(),
                              jinv=(torch.eye(3).reshape(1, 9) + 0.2 * torch.randn(N_WRAP, 9, generator=g)).cuda().contiguous())
    return _CACHE["wrap"]


def test_foreground_many_tiles_equal_one_tile():
    """the 'sdf' pack (8 chunks shorter than 'full') wraps into its own chunks 0 and 1 and the folded colour pack into its own: one launch in which
    every workgroup runs two or three tiles against launches of at most one tile per workgroup"""
    from multiply_amd import hip
    S = wrap_scene()
    imp, ren = S["m"].foreground_implicit_network_list[0], S["m"].foreground_rendering_network_list[0]
    run = lambda a, b: hip.shade_points(imp, ren, S["x"][a:b].contiguous(), S["jinv"][a:b].contiguous(), S["cond"],
                                        mode="reverse", fold=True)
    got = run(0, N_WRAP)
    parts = [run(a, b) for a, b in chunks(N_WRAP, WG * 256)]
    for i, name in enumerate(("sdf", "normal", "rgb")):
        want = torch.cat([p[i] for p in parts])
        assert torch.isfinite(want).all() and float(want.std()) > 0, name
        assert torch.equal(got[i], want), name


def test_background_many_tiles_equal_one_tile():
    """a tile is 8 rays: the shorter density pack hands the ring to the folded colour pack and back, two or three tiles per
    workgroup with a partial last tile"""
    from multiply_amd import hip
    m = wrap_scene()["m"]
    rays = 8 * WG * 2 + 8 * 77 + 5
    d, cam = W.bg_rays(rays, 4100)
    d, cam = d.float().cuda().contiguous(), cam.float().cuda()
    g = torch.Generator().manual_seed(5)
    z = (torch.rand(rays, 32, generator=g) * (1.0 / 3.0)).sort(dim=1, descending=True).values.cuda().contiguous()
    code = m.frame_latent_encoder.weight[W.FRAME].detach().float()
    run = lambda a, b: hip.background(m.bg_implicit_network, m.bg_rendering_network, d[a:b].contiguous(), cam,
                                      z[a:b].contiguous(), code, fold=True)
    got = run(0, rays)
    want = torch.cat([run(a, b) for a, b in chunks(rays, 8 * WG)])
    assert torch.isfinite(want).all() and float(want.std()) > 0
    assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- frame level
def test_frame_against_the_oracle():
    """the 15 x 15 scene of tests/test_render_gpu.py through Multiply.forward (folded: the default) against the oracle: TOL.EVAL;
    the unfolded renderer on the same frame is printed beside it"""
    from tests.test_render_gpu import build, report
    model, oracle, inp = build(H=15, W=15)
    assert model.feature_fold
    R = inp["uv"].shape[1]
    hit = [torch.arange(R), torch.arange(R)]
    want = oracle.forward_eval(inp, hit)
    gin = {**{k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}, "hit_index": hit}
    keys = ("acc_map", "acc_person_list", "rgb_values", "fg_rgb_values", "normal_values")
    outs = {}
    for fold in (True, False):
        model.feature_fold = fold
        got = model(gin)
        torch.cuda.synchronize()
        tag = "folded" if fold else "unfolded"
        outs[fold] = {k: got[k].clone() for k in keys}
        st = {k: report(f"15x15 {tag} {k}", got[k], want[k]) for k in keys}
        st["bg_rgb"] = report(f"15x15 {tag} bg_rgb", model._last["bg_rgb"], want["bg_rgb"])
        if fold:
            for k in st:
                assert TOL.within(st[k], TOL.EVAL[k]), k
    # only the colours move: the geometry outputs do not read the features
    assert torch.equal(outs[True]["normal_values"], outs[False]["normal_values"])
    assert torch.equal(outs[True]["acc_map"], outs[False]["acc_map"])
