"""A point's outputs do not depend on how many tiles its workgroup ran.

The phase-separated MLP kernels keep ONE weight stream per persistent workgroup: the ring is filled once, the DMA wraps from a
pack's last chunk into the first chunks of the pack that runs next, and ids / positions are fetched a tile ahead
(csrc/mlp_core.hpp RingStream, csrc/mlp.hip TileInputs).  None of that may change what is computed per point, so everything here
is torch.equal: one call in which every workgroup of the 256-workgroup grid runs 3-4 tiles (N = 3 * 65536 + 77: some run one tile
fewer, the last tile is partial) against calls small enough that every workgroup runs exactly one tile and never wraps.  Weights:
the "trained" regime of tests/weight_regimes.py -- units in transition, so a stale sigmoid, table entry or staging row cannot hide
behind a saturated value.

The sdf queries come in the three precisions the sampler can run: mp_mlp_sdf ('f16'), mp_mlp_sdf_x2 ('f16x2') and the near-fp32
query the shipped configuration resolves to, mp_tf_sdf_val ('bf16x3').  The last lives in csrc/tfuse.hip and keeps its own per-tile
prologue (the training kernels are not part of the continuous stream); it is checked here all the same, because it is what the
flagship frame's sampler calls.  The background test compares the lane-parallel compositing with itself across tile counts; that it
equals the former serial loop bit for bit is what tools/lib_output_diff.py checks between two builds of the library."""
import ctypes as C

import pytest
import torch

from tests import weight_regimes as W

pytestmark = pytest.mark.gpu

WG = 256                      # persistent grid (csrc/mlp.hip grid_for)
N = 3 * 65536 + 77
SENTINEL = -12345.0
SDF_MODES = ["f16", "f16x2", "bf16x3"]
_S = {}


def scene():
    if not _S:
        m, _, _ = W.regime_networks("trained", 0)
        m.cuda()
        lo, hi = W.canonical_bounds()
        g = torch.Generator().manual_seed(77)
        _S.update(m=m, imp=m.foreground_implicit_network_list[0], ren=m.foreground_rendering_network_list[0],
                  x=W.region_points(N, 7001, lo, hi).float().cuda().contiguous(),
                  x_other=W.region_points(N, 7002, lo, hi).float().cuda().contiguous(),
                  cond=W.pose_vector(3000).float().cuda(),
                  jinv=(torch.eye(3).reshape(1, 9) + 0.2 * torch.randn(N, 9, generator=g)).cuda().contiguous(),
                  perm=torch.randperm(N, generator=g).int().cuda())
    return _S


def chunks(n, step):
    return [(a, min(a + step, n)) for a in range(0, n, step)]


# ---------------------------------------------------------------------------------------------------------------- raw launches
def sdf_launch(mode, x, worklist=None, count=None, max_count=None, out=None):
    from multiply_amd import hip
    S = scene()
    n = x.shape[0] if max_count is None else max_count
    out = torch.empty(x.shape[0], device="cuda") if out is None else out
    if mode == "bf16x3":     # the sampler's near-fp32 query (ray_sampler.py, sampler_sdf_mode 'bf16x3'): csrc/tfuse.hip
        from multiply_amd import train as T
        fs = T.fused_sdf_state(S["imp"]).refresh(S["cond"])
        hip.lib().mp_tf_sdf_val(fs.wpack, fs.bias_all, x, worklist, count, n, out, hip.stream())
        return out
    pk = hip.packed(S["imp"], "sdf", 2)
    pk.refresh(S["cond"])
    fn = {"f16": hip.lib().mp_mlp_sdf, "f16x2": hip.lib().mp_mlp_sdf_x2}[mode]
    fn(C.byref(pk.net), pk.wpack, pk.bias, x, worklist, count, n, out, hip.stream())
    return out


def shade_launch(x, jinv, worklist=None, count=None, max_count=None, seg=None, fill=None):
    """(sdf, normal, rgb) through mp_mlp_shade_rev + mp_mlp_color; outputs pre-filled with `fill` when given"""
    from multiply_amd import hip
    S = scene()
    pki = hip.packed(S["imp"], "full", 2)
    pki.refresh(S["cond"])
    pkr = hip.packed(S["ren"], "color", 2)
    pkr.refresh(hip.pose_embed(S["ren"])(S["cond"]))
    gn = hip.grad_net(S["imp"])
    n = x.shape[0] if max_count is None else max_count
    mk = (lambda *s: torch.full(s, fill, device="cuda")) if fill is not None else (lambda *s: torch.empty(*s, device="cuda"))
    sdf, nrm, rgb = mk(x.shape[0]), mk(x.shape[0], 3), mk(x.shape[0], 3)
    feat = torch.empty(hip.feat_frag_bytes(n), dtype=torch.uint8, device="cuda")
    buf, seg_default = hip.sig_scratch(x.device, n)
    seg = seg_default if seg is None else seg
    # the sweeps address the stored sigmoids by tile WITHIN a segment: a segment longer than the call needs the call's tiles only
    assert buf.numel() >= min(seg, (n + 255) // 256 * 256) * int(hip.lib().mp_sig_bytes_per_point())
    L = hip.lib()
    L.mp_mlp_shade_rev(C.byref(pki.net), pki.wpack, pki.bias, C.byref(gn.pk.net), gn.pk.wpack, gn.w8, x, jinv, worklist, count, n,
                       sdf, nrm, feat, buf, seg, hip.stream())
    L.mp_mlp_color(C.byref(pkr.net), pkr.wpack, pkr.bias, x, nrm, feat, worklist, count, n, rgb, hip.stream())
    return sdf, nrm, rgb


def shade_one_tile_per_wg(x, jinv):
    parts = [shade_launch(x[a:b].contiguous(), jinv[a:b].contiguous()) for a, b in chunks(x.shape[0], WG * 256)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def ref(key, fn):
    """the one-tile-per-workgroup results: computed once, shared by the tests, never written to"""
    if key not in _S:
        _S[key] = fn()
    return _S[key]


def ref_sdf(mode):
    S = scene()
    step = WG * (256 if mode == "f16" else 128)    # the split-activation and the near-fp32 kernels' tile is 128 points
    return ref("sdf_" + mode, lambda: torch.cat([sdf_launch(mode, S["x"][a:b].contiguous()) for a, b in chunks(N, step)]))


def ref_shade():
    S = scene()
    return ref("shade", lambda: shade_one_tile_per_wg(S["x"], S["jinv"]))


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("mode", SDF_MODES)
def test_sdf_many_tiles_equal_one_tile(mode):
    S = scene()
    got = sdf_launch(mode, S["x"])
    want = ref_sdf(mode)
    assert torch.isfinite(want).all() and float(want.std()) > 0
    assert torch.equal(got, want)


def test_shading_many_tiles_equal_one_tile():
    S = scene()
    got = shade_launch(S["x"], S["jinv"])
    want = ref_shade()
    for name, g, w in zip(("sdf", "normal", "rgb"), got, want):
        assert torch.isfinite(w).all() and float(w.std()) > 0, name
        assert torch.equal(g, w), name


# ---------------------------------------------------------------------------------------------------------------- B
def worklist_case():
    S = scene()
    n_in = N - (2 * 256 + 100)      # ends inside a tile; the two tiles behind it are empty
    return S["perm"], torch.tensor([n_in], dtype=torch.int32, device="cuda"), S["perm"][:n_in].long(), S["perm"][n_in:].long()


@pytest.mark.parametrize("mode", SDF_MODES)
def test_sdf_worklist_and_device_count(mode):
    S = scene()
    wl, count, inside, outside = worklist_case()
    out = torch.full((N,), SENTINEL, device="cuda")
    sdf_launch(mode, S["x"], wl, count, N, out)
    assert torch.equal(out[inside], ref_sdf(mode)[inside])
    assert bool((out[outside] == SENTINEL).all())


def test_shading_worklist_and_device_count():
    S = scene()
    wl, count, inside, outside = worklist_case()
    got = shade_launch(S["x"], S["jinv"], wl, count, N, fill=SENTINEL)
    for name, g, w in zip(("sdf", "normal", "rgb"), got, ref_shade()):
        assert torch.equal(g[inside], w[inside]), name
        assert bool((g[outside] == SENTINEL).all()), name


# ---------------------------------------------------------------------------------------------------------------- C
def test_shading_segment_boundaries():
    """segments of 5 tiles (offsets != 0, every workgroup at most one tile) against one segment"""
    S = scene()
    small = shade_launch(S["x"], S["jinv"], seg=256 * 5)
    big = shade_launch(S["x"], S["jinv"], seg=1 << 21)
    for name, g, w in zip(("sdf", "normal", "rgb"), small, big):
        assert torch.equal(g, w), name
    for name, g, w in zip(("sdf", "normal", "rgb"), small, ref_shade()):
        assert torch.equal(g, w), name


# ---------------------------------------------------------------------------------------------------------------- D
def test_grad_first_tiles_do_not_see_later_tiles():
    """two inputs that agree on every workgroup's FIRST tile and differ behind it: the first tiles' outputs are bit-equal (a
    table, staging row or prefetched position of the wrong tile would show)"""
    S = scene()
    first = WG * 256
    x2 = S["x_other"].clone()
    x2[:first] = S["x"][:first]
    a = ref_shade()
    b = shade_launch(x2, S["jinv"])
    for name, u, v in zip(("sdf", "normal", "rgb"), a, b):
        assert torch.equal(u[:first], v[:first]), name
    assert not torch.equal(a[1][first:], b[1][first:])


# ---------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("rays", [8 * WG * 2 + 8 * 77 + 5, 8 * WG + 3])
def test_background_many_tiles_equal_one_tile(rays):
    """a tile is 8 rays: more than 2 tiles per workgroup with a partial last tile; one full round plus a partial tile"""
    from multiply_amd import hip
    S = scene()
    m = S["m"]
    d, cam = W.bg_rays(rays, 4100)
    d, cam = d.float().cuda().contiguous(), cam.float().cuda()
    g = torch.Generator().manual_seed(5)
    z = (torch.rand(rays, 32, generator=g) * (1.0 / 3.0)).sort(dim=1, descending=True).values.cuda().contiguous()
    code = m.frame_latent_encoder.weight[W.FRAME].detach().float()
    run = lambda a, b: hip.background(m.bg_implicit_network, m.bg_rendering_network, d[a:b].contiguous(), cam, z[a:b].contiguous(), code)
    got = run(0, rays)
    want = torch.cat([run(a, b) for a, b in chunks(rays, 8 * WG)])
    assert torch.isfinite(want).all() and float(want.std()) > 0
    assert torch.equal(got, want)
