"""The deterministic forms of the three small sums of a training step:
  * the last layer's 256 + 1 sums of the fused SDF / background backward (csrc/tfuse.hip: mp_tf_sdf_bwd_det, mp_tf_bg_bwd_det),
  * d beta of the two compositing adjoints (csrc/composite.hip: mp_tr_composite_bwd_det, mp_tr_composite_geometry_bwd_det),
  * d tfs of the canonical warp's adjoint (csrc/train.hip: mp_tr_warp_bwd_det).
Every one: two launches give the same bits (torch.equal); the fused sums agree with the atomic form within the bound
tests/test_train_gpu.py::test_fused_sdf_kernels_against_autograd holds that tensor to against the layer-wise path (2e-4 of the
tensor's maximum); d beta and d tfs are within c 2^-24 sum |terms| of a float64 sum of the same per-point terms, c from
tests/tolerances_deterministic.py (twice what the atomic kernel needs on the same inputs)."""
import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import geometry_train_reference as GT
from tests import tolerances_deterministic as TOLD
from tests import train_elementwise_reference as R
from tests.util import seeded_networks

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FUSED_REL = 2e-4      # test_fused_sdf_kernels_against_autograd: every parameter gradient, fused against layer-wise


def _rel(got, want):
    got, want = got.double().cpu(), want.double().cpu()
    return (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)


# =========================================================================================================== fused backward sums
# The grid of both kernels is the number of 128-point tiles (csrc/tfuse.hip: dim3((P + 127) / 128)): a workgroup runs exactly ONE
# tile, whatever P, so "a workgroup with two tiles" does not exist here and a workgroup's row is a pure function of the grid.  What
# does change with P is the finishing pass: up to 64 rows are added by one launch, more by two levels (runs of 64 rows, then the
# runs): 8321 points = 66 tiles takes the second path.
FUSED_P = (300, 66 * 128 - 127)


def _fused_setup(kind, P):
    from multiply_amd import train as T
    m, _ = seeded_networks(1, 0)                     # the geometric initialisation
    m = m.cuda()
    torch.manual_seed(31 + P)
    if kind == "sdf":
        net = m.foreground_implicit_network_list[0]
        x = (torch.rand(P, 3, device="cuda") - 0.5) * 1.6
        ev = T.ImplicitTrainFused(net, x, torch.randn(69, device="cuda") * 0.1)
        L, st = T.hip.lib(), T.hip.stream()
        dgrad = torch.randn(P, 3, device="cuda")     # the gradient sweep's upstream -> dG in the arena, as backward() does
        L.mp_tr_pe_grad_bwd(ev.x, P, net.multires, dgrad, T.off(ev.arena, ev.o_G), ev.E, T.off(ev.arena, ev.o_dG), ev.E, None, st)
        w8 = ev.w8
    else:
        net = m.bg_implicit_network
        d = torch.nn.functional.normalize(torch.randn(P, 3, device="cuda"), dim=1)
        x = torch.cat([d, torch.rand(P, 1, device="cuda")], 1).contiguous()
        ev = T.ImplicitTrainFusedBG(net, x, torch.randn(32, device="cuda") * 0.1)
        w8 = ev.lins[8].W
    dfeat, dsdf = torch.randn(P, 256, device="cuda"), torch.randn(P, device="cuda")
    return T, ev, w8, dfeat, dsdf


def _fused_launch(T, kind, ev, w8, P, dfeat, dsdf, det):
    L, st = T.hip.lib(), T.hip.stream()
    out = torch.zeros(257, device="cuda")            # dw8 [256], db8 [1]
    if det:
        part = T._part(L.mp_tf_bwd_part_floats, P)
        part.fill_(float("nan"))                     # every row the finishing pass reads must have been written
        fn = L.mp_tf_sdf_bwd_det if kind == "sdf" else L.mp_tf_bg_bwd_det
        fn(ev.fs.wpack, w8, ev.arena, P, dfeat, dsdf, out, T.off(out, 256), part, st)
    else:
        fn = L.mp_tf_sdf_bwd if kind == "sdf" else L.mp_tf_bg_bwd
        fn(ev.fs.wpack, w8, ev.arena, P, dfeat, dsdf, out, T.off(out, 256), st)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("P", FUSED_P)
@pytest.mark.parametrize("kind", ["sdf", "bg"])
def test_fused_backward_sums(kind, P):
    T, ev, w8, dfeat, dsdf = _fused_setup(kind, P)
    tiles = (P + 127) // 128
    assert (P, tiles) in ((300, 3), (8321, 66)) and P % 128 != 0          # a ragged last tile; 66 > 64 rows: two finishing levels
    atomic = _fused_launch(T, kind, ev, w8, P, dfeat, dsdf, det=False)
    stash = ev.arena.clone()
    d1 = _fused_launch(T, kind, ev, w8, P, dfeat, dsdf, det=True)
    assert torch.equal(ev.arena.view(torch.int32), stash.view(torch.int32)), "the deterministic form leaves the same stashes behind"
    d2 = _fused_launch(T, kind, ev, w8, P, dfeat, dsdf, det=True)
    assert torch.isfinite(d1).all() and torch.equal(d1, d2)
    e_w, e_b = _rel(d1[:256], atomic[:256]), _rel(d1[256:], atomic[256:])
    print(f"[deterministic sums] fused {kind} P {P}: dw8 {e_w:.3e}, db8 {e_b:.3e} of the atomic form's maximum")
    assert e_w < FUSED_REL and e_b < FUSED_REL


# ========================================================================================================================= d beta
N_RAYS, N_PERSON, N_Z = 70, 2, 17                    # 16 samples per ray and person
BETA, LEVEL = 0.02, 0.5


def _composite_inputs():
    hits = [np.arange(0, 50), np.arange(30, 65)]     # rays hit by none, one and both persons
    inv, z, sdf = G.ragged_case(N_RAYS, N_PERSON, N_Z, seed=4, hits=hits)
    rs = np.random.RandomState(9)
    rgb = [rs.rand(s.shape[0], s.shape[1], 3).astype(np.float32) for s in sdf]
    up = dict(rgb=rs.randn(N_RAYS, 3).astype(np.float32), acc=rs.randn(N_RAYS).astype(np.float32),
              accp=rs.randn(N_RAYS, N_PERSON).astype(np.float32), bg=rs.rand(N_RAYS, 3).astype(np.float32))
    return inv, z, sdf, rgb, up


def _dbe(s, beta):
    """d sigma / d beta of the Laplace density (tests/geometry_train_reference.adjoint_formulas), float64"""
    eab = np.exp(-np.abs(s) / beta)
    return np.where(s > 0, 0.5 / beta**2 * eab * (s / beta - 1), np.where(s < 0, -1 / beta**2 + 0.5 / beta**2 * eab * (1 + s / beta), -0.5 / beta**2))


def _composite_terms64(inv, z, sdf, rgb, up):
    """float64: the per-sample terms d sigma_i (d sigma_i / d beta) of mp_composite's adjoint -> (their sum, the sum of their
    magnitudes).  Samples of a ray merged by (t_end, person); rgb_values = sum w rgb + T_bg bg with T_bg the transmittance in front of
    the ray's last merged sample; acc = sum w; acc_person = the persons' shares."""
    beta = float(np.float32(BETA))
    tot = mag = 0.0
    for r in range(N_RAYS):
        ps = [n for n in range(N_PERSON) if inv[n][r] >= 0]
        if not ps:
            continue
        key = sorted((float(z[n][inv[n][r], i + 1]), n, i) for n in ps for i in range(N_Z - 1))
        who, idx = np.array([k[1] for k in key]), np.array([k[2] for k in key])
        row = {n: int(inv[n][r]) for n in ps}
        s = np.array([float(sdf[n][row[n], i]) for _, n, i in key])
        dt = np.array([float(z[n][row[n], i + 1]) - float(z[n][row[n], i]) for _, n, i in key])
        c = np.array([rgb[n][row[n], i].astype(np.float64) for _, n, i in key])
        fe = G.laplace_density(s, beta) * dt
        E = np.cumsum(fe) - fe
        w = (1 - np.exp(-fe)) * np.exp(-E)
        dC = up["rgb"][r].astype(np.float64)
        dw = c @ dC + float(up["acc"][r]) + up["accp"][r].astype(np.float64)[who]
        behind = np.cumsum((dw * w)[::-1])[::-1] - dw * w
        dfe = dw * np.exp(-E) * np.exp(-fe) - behind
        Tbg = np.exp(-E[-1])
        dfe[:-1] -= float(dC @ up["bg"][r].astype(np.float64)) * Tbg          # T_bg depends on every sample but the last
        t = dfe * dt * _dbe(s, beta)
        tot += t.sum()
        mag += np.abs(t).sum()
    return tot, mag


def _geometry_terms64(inv, z, sdf, ups):
    """the same for mp_composite_geometry's adjoint, from the reference's closed form: its d sdf is d sigma times d sigma / d sdf"""
    beta = float(np.float32(BETA))
    d_sdf, d_beta = GT.adjoint_formulas(N_RAYS, inv, z, sdf, beta, LEVEL, ups)
    mag = 0.0
    for n in range(N_PERSON):
        rows = inv[n][inv[n] >= 0]
        s = sdf[n][rows].astype(np.float64)
        dsig = d_sdf[n][rows] / (-(0.5 / beta**2) * np.exp(-np.abs(s) / beta))
        mag += np.abs(dsig * _dbe(s, beta)).sum()
    return d_beta, mag


def _composite_launch(kind, det, inv, z, sdf, rgb, up, ups):
    from multiply_amd import hip
    L, st = hip.lib(), hip.stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [[dev(a) for a in inv], [dev(a) for a in z], [dev(a.reshape(-1)) for a in sdf], [dev(a.reshape(-1, 3)) for a in rgb]]
    tabs = [hip.device_ints([t.data_ptr() for t in ts], "cuda") for ts in keep]
    d_sdf = [torch.zeros(a.size, device="cuda") for a in sdf]
    d_rgb = [torch.zeros(a.size // 3, 3, device="cuda") for a in rgb]
    t_dsdf, t_drgb = (hip.device_ints([t.data_ptr() for t in ts], "cuda") for ts in (d_sdf, d_rgb))
    beta = torch.tensor([BETA], dtype=torch.float32, device="cuda")
    d_beta = torch.zeros(1, device="cuda")
    part = torch.full((N_RAYS,), float("nan"), device="cuda")
    tail = (part, st) if det else (st,)
    if kind == "composite":
        g = [dev(up[k]) for k in ("rgb", "acc", "accp")]
        fn = L.mp_tr_composite_bwd_det if det else L.mp_tr_composite_bwd
        fn(N_RAYS, N_PERSON, N_Z, *tabs, beta, dev(up["bg"]), *g, t_dsdf, t_drgb, torch.zeros(N_RAYS, 3, device="cuda"), d_beta, *tail)
    else:
        g = [dev(np.asarray(ups[k], dtype=np.float32)) for k in GT.DIFF_KEYS]
        fn = L.mp_tr_composite_geometry_bwd_det if det else L.mp_tr_composite_geometry_bwd
        fn(N_RAYS, N_PERSON, N_Z, *tabs[:3], beta, LEVEL, *g, t_dsdf, d_beta, *tail)
    torch.cuda.synchronize()
    return d_beta.cpu(), [t.cpu() for t in d_sdf]


@pytest.mark.parametrize("kind", ["composite", "geometry"])
def test_d_beta(kind):
    inv, z, sdf, rgb, up = _composite_inputs()
    ups = None
    if kind == "composite":
        want, mag = _composite_terms64(inv, z, sdf, rgb, up)
    else:
        ref = G.geometry_reference(N_RAYS, inv, z, sdf, BETA, LEVEL)
        rs = np.random.RandomState(104)
        ups = dict(depth=rs.randn(N_RAYS), depth_person=rs.randn(N_RAYS, N_PERSON), acc_solo=rs.randn(N_RAYS, N_PERSON),
                   depth_solo=rs.randn(N_RAYS, N_PERSON), depth_solo_level=rs.randn(N_RAYS, N_PERSON))
        ups = {k: v.astype(np.float32) for k, v in ups.items()}
        ups["depth_solo_level"][G.exempt(ref["fe_cross_solo"], ref["margin_solo"])] = 0.0
        want, mag = _geometry_terms64(inv, z, sdf, ups)
    assert mag > 0 and np.isfinite(want)
    c_atomic = max(abs(float(_composite_launch(kind, False, inv, z, sdf, rgb, up, ups)[0]) - want) / (U * mag) for _ in range(3))
    b1, s1 = _composite_launch(kind, True, inv, z, sdf, rgb, up, ups)
    b2, s2 = _composite_launch(kind, True, inv, z, sdf, rgb, up, ups)
    assert torch.equal(b1, b2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
    s0 = _composite_launch(kind, False, inv, z, sdf, rgb, up, ups)[1]
    assert all(torch.equal(a, b) for a, b in zip(s1, s0)), "d sdf never went through atomics: the two forms agree bit for bit"
    c_det = abs(float(b1) - want) / (U * mag)
    print(f"[deterministic sums] d beta ({kind}): |err| / (2^-24 sum |terms|): atomic {c_atomic:.3f}, deterministic {c_det:.3f}; "
          f"d beta {want:.6e}, sum |terms| {mag:.6e}")
    assert c_det <= TOLD.C_D_BETA[kind]


# ========================================================================================================================== d tfs
def _warp_terms64(inp, with_dj):
    """float64 per-point terms w_j dT_k (+ wc_j dRc_k) of the float32 inputs -> (their sums [24][12], the sums of their magnitudes)"""
    n = inp["xc"].shape[0]
    tfs = inp["tfs"].double().view(R.NJ, 4, 4)
    w, wc = inp["skin_w"].double()[inp["nn_posed"]], inp["skin_w"].double()[inp["nn_cano"]]
    Rm = torch.einsum("ij,jab->iab", w, tfs[:, :3, :3])
    u = torch.einsum("iba,ib->ia", torch.linalg.inv(Rm), inp["dxc"].double())              # R^-T dx_c
    dT = torch.cat([-u[:, :, None] * inp["xc"].double()[:, None, :], -u[:, :, None]], 2)     # [n][3][4]
    terms = w[:, :, None, None] * dT[:, None]                                                 # [n][24][3][4]
    tot, mag = terms.sum(0), terms.abs().sum(0)
    if with_dj:
        M, dM = inp["jinv"].double().view(n, 3, 3), inp["djinv"].double().view(n, 3, 3)
        dRc = -M.transpose(1, 2) @ dM @ M.transpose(1, 2)
        t2 = wc[:, :, None, None] * dRc[:, None]
        tot[:, :, :3] += t2.sum(0)
        mag[:, :, :3] += t2.abs().sum(0)
    return tot.reshape(R.NJ, 12), mag.reshape(R.NJ, 12)


def _warp_launch(inp, with_dj, det):
    from multiply_amd import hip, train as T
    L, st = hip.lib(), hip.stream()
    n = inp["xc"].shape[0]
    cu = lambda t: t.contiguous().cuda()
    a = [cu(inp["xc"]), cu(inp["dxc"]), cu(inp["jinv"]), cu(inp["djinv"]) if with_dj else None, cu(inp["nn_posed"].to(torch.int32)),
         cu(inp["nn_cano"].to(torch.int32)), n, cu(inp["skin_w"]), cu(inp["tfs"])]
    dtfs = torch.zeros(R.NJ, 16, device="cuda")
    if det:
        part = T._part(L.mp_tr_warp_bwd_part_floats, n)
        part.fill_(float("nan"))
        L.mp_tr_warp_bwd_det(*a, dtfs, part, st)
    else:
        L.mp_tr_warp_bwd(*a, dtfs, st)
    torch.cuda.synchronize()
    return dtfs.cpu()


@pytest.mark.parametrize("with_dj", [True, False])
def test_d_tfs(with_dj):
    n = 700                                          # three runs of 256 points, the last ragged
    inp = R.case_warp(n, 9700, with_dj)
    want, mag = _warp_terms64(inp, with_dj)
    ratio = lambda got: float(((got[:, :12].double() - want).abs() / (U * mag).clamp_min(1e-300))[mag > 0].max())
    c_atomic = max(ratio(_warp_launch(inp, with_dj, False)) for _ in range(3))
    d1, d2 = _warp_launch(inp, with_dj, True), _warp_launch(inp, with_dj, True)
    assert torch.equal(d1, d2) and bool((d1[:, 12:] == 0).all())
    assert bool((d1[:, :12][mag == 0] == 0).all()), "an entry no point contributes to stays zero"
    c_det = ratio(d1)
    print(f"[deterministic sums] d tfs (djinv {with_dj}): max |err| / (2^-24 sum |terms|): atomic {c_atomic:.3f}, deterministic {c_det:.3f}")
    assert c_det <= TOLD.C_D_TFS[with_dj]
