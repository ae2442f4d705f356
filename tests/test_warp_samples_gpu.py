"""The blend table and the canonical warp on IMPLICIT samples (csrc/geom.hip: mp_blend_table, mp_warp_inverse with its worklist and
the binned training walk, mp_warp_inverse_shade, the need-flag form of mp_warp_jacobian) through the C ABI against the float64
reference (oracle/geom_oracle64.py).  Scene: tests/geom_scene.py; its conditions: tests/test_geom_oracle64_cpu.py.  Every output is
pre-filled with a sentinel; every equality, set and "untouched" assertion is exact; x_c, the table and jinv are bounded by
tolerances.GEOM64."""
import numpy as np
import pytest
import torch

from oracle import geom_oracle64 as R
from tests import geom_scene as G
from tests import tolerances as TOL

pytestmark = pytest.mark.gpu

F_SENT, B_SENT, I_SENT = -55.0, 90, -7
K, NS, ZS, S = G.K_WARP, G.NS, G.ZSTRIDE, G.S_SHADE
CUT = 37                      # rays behind the device count in the reduced-count cases
V = 6890


def err(name, got, want):
    e = (got.double() - want.double()).abs().max().item() if got.numel() else 0.0
    print(f"[geom64] {name}: max abs err {e:.3e}")
    return e


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def w(smpl_tables):
    """the warp scene: K hit rays of mp_ray_cull, their depth tables, and the float64 reference of both point sets (computed once)"""
    sc = G.device_scene(smpl_tables)
    hit, count, _ = G.ray_cull(sc, sc["obb"], G.R_FULL, 0)
    ids = G.pick_rays(hit[:count])
    assert ids.numel() == K and (ids[1:] > ids[:-1]).all()
    d = dict(sc)
    d["ids"] = ids.cuda()
    d["hit_index"] = ids.to(torch.int32).cuda()
    d["dirs_hit"] = sc["dirs"][d["ids"]]
    d["tab64"] = R.blend_table64(sc["skin_w"], sc["tfs"])
    for key, z, n_s in (("smp", G.sampler_depths(), NS), ("shd", G.shade_depths(), S)):
        x64 = G.sample_points(sc["cam"], d["dirs_hit"], z.cuda(), n_s)
        d2, nn, gap = R.nearest_vertex64(x64, sc["verts"])
        d[key] = dict(z=z.cuda().contiguous(), x64=x64, d2=d2, nn=nn, gap=gap, out=R.outlier64(d2),
                      band=(d2.sqrt() - 0.1).abs() < 1e-6, unsure=gap <= G.d2_eval_bound(d2))
        n = x64.shape[0]
        print(f"[geom64] {key}: {n} points, {int(d[key]['out'].sum())} outliers, {int(d[key]['band'].sum())} on the outlier radius, "
              f"{int(d[key]['unsure'].sum())} with a runner-up inside the fp32 evaluation error")
        # the conditions of the comparisons below, by the reference alone.  (`unsure` points -- mostly samples far in front of or
        # behind the body, which see many vertices about equally far -- are not left out: check_x_c compares them with every vertex
        # that is a correct answer)
        assert int(d[key]["band"].sum()) <= 0.001 * n and int(d[key]["unsure"].sum()) <= 0.005 * n
        assert 0.03 * n < int((~d[key]["out"]).sum()) < 0.5 * n
    return d


def count_tensor(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def run_warp(w, z, z_stride, n_s, mode, *, hit_index=None, n_hit=None, max_rays=K, ray_active=None, launch_active=None, binned=False,
             pose=None, dirs=None):
    """mp_warp_inverse on implicit samples -> sentinel-filled outputs"""
    from multiply_amd import hip
    L = hip.lib()
    n = max_rays * n_s
    o = dict(xc=torch.full((n + 16, 3), F_SENT, device="cuda"), outlier=torch.full((n + 16,), B_SENT, dtype=torch.uint8, device="cuda"),
             sdf=torch.full((n + 16,), F_SENT, device="cuda"), worklist=torch.full((n + 16,), I_SENT, dtype=torch.int32, device="cuda"),
             work_count=torch.zeros(2, dtype=torch.int32, device="cuda"))
    bw = torch.empty(int(L.mp_warp_bin_work_bytes(n)), dtype=torch.uint8, device="cuda") if binned else None
    L.mp_warp_inverse(None, w["dirs"] if dirs is None else dirs, w["pose_d"] if pose is None else pose,
                      w["hit_index"] if hit_index is None else hit_index, count_tensor(max_rays if n_hit is None else n_hit), z, z_stride,
                      n_s, max_rays, w["vsorted"], w["cbound"], w["btab"], mode, ray_active, launch_active, o["xc"], o["outlier"], o["sdf"],
                      o["worklist"], o["work_count"], bw, hip.stream())
    torch.cuda.synchronize()
    o["n"] = n
    for k in ("xc", "outlier", "sdf"):
        assert (o[k][n:] == (B_SENT if k == "outlier" else F_SENT)).all(), f"{k} written behind the last point"
    assert int(o["work_count"][1]) == 0
    return o


def worklist_ids(o):
    c = int(o["work_count"][0])
    assert 0 <= c <= o["n"]
    assert (o["worklist"][c:] == I_SENT).all(), "worklist written behind its count"
    ids = o["worklist"][:c].long()
    assert ids.unique().numel() == c, "duplicate ids in the worklist"
    return torch.sort(ids).values


def untouched(o, pmask):
    """the points of pmask kept their sentinels in every per-point output"""
    return bool((o["xc"][:o["n"]][pmask] == F_SENT).all() and (o["outlier"][:o["n"]][pmask] == B_SENT).all() and
                (o["sdf"][:o["n"]][pmask] == F_SENT).all())


def equal_on(a, b, pmask):
    n = a["n"]
    return all(same_bits(a[k][:n][pmask], b[k][:n][pmask]) for k in ("xc", "outlier", "sdf"))


def check_x_c(tag, w, ref, xc, written):
    """x_c = I (x - c) of the float64 nearest vertex.  mp_warp_inverse does not say which vertex it took: where the runner-up lies
    within the fp32 evaluation error of the kernel's distance arithmetic (tests/geom_scene.py d2_eval_bound) x_c must be that of ONE
    of the vertices that near; everywhere else (>= 99.5 % of the points) it is compared with the argmin's"""
    sel = written & ~ref["unsure"]
    assert int(sel.sum()) >= 0.995 * int(written.sum())
    want = R.warp64(ref["x64"][sel], ref["nn"][sel], w["tab64"])
    assert err(f"{tag} ({int(sel.sum())} points)", xc[sel], want) < TOL.GEOM64["x_c"]
    idx = torch.nonzero(written & ref["unsure"]).reshape(-1)
    if idx.numel():
        x = ref["x64"][idx]
        d2 = ((x[:, None, :] - w["verts"].double()[None]) ** 2).sum(-1)
        dk, ik = torch.topk(d2, 8, dim=1, largest=False)
        allowed = dk - dk[:, :1] <= G.d2_eval_bound(dk[:, :1])
        assert not allowed[:, -1].any()                                       # 8 candidates were enough
        cand = torch.stack([R.warp64(x, ik[:, j], w["tab64"]) for j in range(8)], 1)          # [p][8][3]
        e = (cand - xc[idx].double()[:, None]).abs().amax(-1)
        e = torch.where(allowed, e, torch.full_like(e, float("inf"))).min(1).values
        print(f"[geom64] {tag}: {idx.numel()} points with several admissible vertices, max abs err to the best of them {float(e.max()):.3e}")
        assert float(e.max()) < TOL.GEOM64["x_c"]


def point_mask(ray_mask, n_s):
    return ray_mask[:, None].expand(-1, n_s).reshape(-1)


# ------------------------------------------------------------------------------------------------ blend table
@pytest.mark.parametrize("n_verts", [1, 255, 257, V])
def test_blend_table_matches_float64(w, n_verts):
    from multiply_amd import hip
    tab = torch.full((n_verts + 4, 3, 4), F_SENT, device="cuda")
    hip.lib().mp_blend_table(w["skin_w"], w["tfs"], n_verts, tab, hip.stream())
    torch.cuda.synchronize()
    assert (tab[n_verts:] == F_SENT).all()
    assert err(f"blend table[{n_verts}]", tab[:n_verts], w["tab64"][:n_verts]) < TOL.GEOM64["blend_table"]
    assert same_bits(tab[:n_verts].reshape(-1, 12), w["btab"][:n_verts].reshape(-1, 12))      # a prefix is the same table


# ------------------------------------------------------------------------------------------------ mp_warp_inverse, implicit samples
@pytest.fixture(scope="module")
def base(w):
    """the un-masked, un-binned launches the variants below are compared with"""
    z = w["smp"]["z"]
    return {mode: run_warp(w, z, ZS, NS, mode) for mode in (0, 1)}


@pytest.mark.parametrize("mode", [0, 1])
def test_implicit_samples_match_float64(w, base, mode):
    ref, o = w["smp"], base[mode]
    n = o["n"]
    out = o["outlier"][:n]
    assert ((out == 0) | (out == 1)).all()
    assert torch.equal(out.bool()[~ref["band"]], ref["out"][~ref["band"]]), "outlier flags"
    written = torch.ones(n, dtype=torch.bool, device="cuda") if mode == 0 else out == 0
    if mode == 1:
        assert (o["sdf"][:n][out == 1] == 4.0).all() and (o["sdf"][:n][out == 0] == F_SENT).all()
        assert (o["xc"][:n][out == 1] == F_SENT).all()                       # outliers are skipped
    else:
        assert (o["sdf"][:n] == F_SENT).all()
    check_x_c(f"x_c mode {mode}", w, ref, o["xc"][:n], written)
    # worklist: every active point (mode 0), the non-outliers (mode 1)
    assert torch.equal(worklist_ids(o), torch.nonzero(written).reshape(-1))


@pytest.mark.parametrize("mode,binned", [(0, False), (1, False), (0, True)])
def test_device_count_below_the_bound(w, base, mode, binned):
    o = run_warp(w, w["smp"]["z"], ZS, NS, mode, n_hit=K - CUT, binned=binned)
    tail = point_mask(torch.arange(K, device="cuda") >= K - CUT, NS)
    assert untouched(o, tail) and equal_on(o, base[mode], ~tail)
    assert torch.equal(worklist_ids(o), worklist_ids(base[mode])[worklist_ids(base[mode]) < (K - CUT) * NS])


@pytest.mark.parametrize("mode,binned", [(0, False), (1, False), (0, True)])
def test_ray_active_mask(w, base, mode, binned):
    active = (torch.arange(K, device="cuda") % 3 != 0).to(torch.int32)
    for n_hit in (K, K - CUT):
        o = run_warp(w, w["smp"]["z"], ZS, NS, mode, ray_active=active, n_hit=n_hit, binned=binned)
        on = point_mask((active != 0) & (torch.arange(K, device="cuda") < n_hit), NS)
        assert untouched(o, ~on) and equal_on(o, base[mode], on)
        full = worklist_ids(base[mode])
        assert torch.equal(worklist_ids(o), full[on[full]])


@pytest.mark.parametrize("mode,binned", [(0, False), (1, False), (0, True)])
def test_launch_active_zero_changes_nothing(w, mode, binned):
    off = count_tensor(0)
    o = run_warp(w, w["smp"]["z"], ZS, NS, mode, launch_active=off, binned=binned)
    assert untouched(o, torch.ones(o["n"], dtype=torch.bool, device="cuda"))
    assert int(o["work_count"][0]) == 0 and (o["worklist"] == I_SENT).all()


def test_binned_training_walk_is_the_same_by_id(w, base):
    o = run_warp(w, w["smp"]["z"], ZS, NS, 0, binned=True)
    every = torch.ones(o["n"], dtype=torch.bool, device="cuda")
    assert equal_on(o, base[0], every)
    assert torch.equal(worklist_ids(o), worklist_ids(base[0]))               # a permutation of the same ids
    assert not torch.equal(o["worklist"][:o["n"]], base[0]["worklist"][:o["n"]])      # (and it did walk in another order)


# ------------------------------------------------------------------------------------------------ the staged worklist's in-loop flush
def _explicit(w, pts, mode):
    """the same points as explicit pts, in chunks of 4096 slabs: one slab per wave, nothing staged across slabs"""
    from multiply_amd import hip
    L = hip.lib()
    n = pts.shape[0]
    o = dict(xc=torch.full((n, 3), F_SENT, device="cuda"), outlier=torch.full((n,), B_SENT, dtype=torch.uint8, device="cuda"),
             sdf=torch.full((n,), F_SENT, device="cuda"), n=n)
    chunk = 256 * 16 * 64
    appended = 0
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        wl = torch.full((m,), I_SENT, dtype=torch.int32, device="cuda")
        wc = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.mp_warp_inverse(pts[s:s + m], None, None, None, None, None, 0, 1, m, w["vsorted"], w["cbound"], w["btab"], mode, None, None,
                          o["xc"][s:s + m], o["outlier"][s:s + m], o["sdf"][s:s + m], wl, wc, None, hip.stream())
        appended += int(wc.item())
    torch.cuda.synchronize()
    return o, appended


@pytest.mark.parametrize("mode", [0, 1])
def test_in_loop_flush_of_the_staged_worklist(w, mode):
    """4 100 rays x 520 samples = 33 800 slabs for 256 x 16 waves: more than 8 slabs per wave, so a wave's strip of staged ids (512)
    runs full inside the loop.  Results by id are those of the same points run as explicit points, one slab per wave.  Directions,
    camera and depths sit on dyadic grids (2^-10, 2^-8, 2^-10) that make cam + t d exact in fp32: the explicit points are the
    kernel's own, bit for bit, however it evaluates them."""
    rays, n_s, stride = 4100, 520, 528
    rng = np.random.RandomState(40 + mode)
    q = lambda t, b: torch.round(t * 2.0 ** b) / 2.0 ** b
    dirs_q = q(w["dirs"], 10).contiguous()
    pose_q = q(w["pose_d"], 8).contiguous()
    cam_q = pose_q[[3, 7, 11]]
    if mode == 0:
        pick = torch.arange(rays, device="cuda") % K
        z = G.Z_LO + (torch.arange(n_s)[None] + torch.from_numpy(rng.uniform(0, 1, (rays, 1)))) * ((G.Z_HI - G.Z_LO) / n_s)
    else:
        # depths within 0.05 of the sample nearest to the body, on the rays that come within 0.04 of it: (nearly) all points appended
        ref = w["smp"]
        dmin, smin = ref["d2"].reshape(K, NS).sqrt().min(1)
        close = torch.nonzero(dmin < 0.04).reshape(-1)
        assert close.numel() > 50
        pick = close[torch.arange(rays, device="cuda") % close.numel()]
        t0 = ref["z"][pick, smin[pick]].cpu().double()
        z = t0[:, None] + torch.from_numpy(rng.uniform(-0.05, 0.05, (rays, n_s)))
    zt = torch.full((rays, stride), float("nan"))
    zt[:, :n_s] = q(z.float(), 10)
    zt = zt.cuda().contiguous()
    hit_index = w["hit_index"][pick].contiguous()
    pts64 = cam_q.double()[None, None] + zt[:, :n_s].double()[..., None] * dirs_q[hit_index.long()].double()[:, None]
    pts = pts64.float()
    assert torch.equal(pts.double(), pts64)                                   # exact in fp32
    pts = pts.reshape(-1, 3).contiguous()
    assert -(-rays // 64) * n_s > 256 * 16 * 8                                # more than 8 slabs for some wave of the largest launch
    o = run_warp(w, zt, stride, n_s, mode, hit_index=hit_index, max_rays=rays, pose=pose_q, dirs=dirs_q)
    e, appended = _explicit(w, pts, mode)
    n = o["n"]
    assert same_bits(o["xc"][:n], e["xc"]) and torch.equal(o["outlier"][:n], e["outlier"]) and same_bits(o["sdf"][:n], e["sdf"])
    ids = worklist_ids(o)
    want = torch.arange(n, device="cuda") if mode == 0 else torch.nonzero(o["outlier"][:n] == 0).reshape(-1)
    print(f"[geom64] flush mode {mode}: {ids.numel()} of {n} points appended")
    assert torch.equal(ids, want) and ids.numel() == appended
    assert ids.numel() >= 0.95 * n                                            # enough ids per wave to fill a strip inside the loop


# ------------------------------------------------------------------------------------------------ the shading warp
def run_shade(w, z, eval_mode, beta, *, binned=False):
    from multiply_amd import hip
    L = hip.lib()
    n = K * S
    o = dict(xc=torch.full((n + 16, 3), F_SENT, device="cuda"), outlier=torch.full((n + 16,), B_SENT, dtype=torch.uint8, device="cuda"),
             need=torch.full((n + 16,), B_SENT, dtype=torch.uint8, device="cuda"), sdf=torch.full((n + 16,), F_SENT, device="cuda"),
             nn=torch.full((n + 16,), I_SENT, dtype=torch.int32, device="cuda"),
             worklist=torch.full((n + 16,), I_SENT, dtype=torch.int32, device="cuda"),
             work_count=torch.zeros(2, dtype=torch.int32, device="cuda"), n=n)
    bw = torch.empty(int(L.mp_warp_bin_work_bytes(n)), dtype=torch.uint8, device="cuda") if binned else None
    L.mp_warp_inverse_shade(w["dirs"], w["pose_d"], w["hit_index"], count_tensor(K), z, S + 1, S, K, w["vsorted"], w["cbound"], w["btab"],
                            eval_mode, torch.tensor([beta], dtype=torch.float32, device="cuda"), o["xc"], o["outlier"], o["need"],
                            o["sdf"], o["worklist"], o["work_count"], o["nn"], bw, hip.stream())
    torch.cuda.synchronize()
    for k, s in (("xc", F_SENT), ("outlier", B_SENT), ("need", B_SENT), ("sdf", F_SENT), ("nn", I_SENT)):
        assert (o[k][n:] == s).all(), f"{k} written behind the last point"
    return o


def check_nearest(tag, x64, verts, d2, nn64, nn_k, sel):
    """the kernel's vertex on the points of sel: the float64 argmin, or a vertex as near within the fp32 evaluation error"""
    took = ((x64[sel] - verts.double()[nn_k[sel].long()]) ** 2).sum(-1)
    same = nn_k[sel].long() == nn64[sel]
    print(f"[geom64] {tag}: {int(same.sum())} of {int(sel.sum())} points took the float64 argmin")
    assert (same | (took - d2[sel] <= G.d2_eval_bound(d2[sel]))).all(), f"{tag}: a vertex that is not the nearest"
    assert int(same.sum()) >= 0.999 * int(sel.sum())


def check_shade_points(tag, w, ref, o, flagged):
    n = o["n"]
    assert ((o["nn"][:n][flagged] >= 0) & (o["nn"][:n][flagged] < V)).all()
    check_nearest(tag, ref["x64"], w["verts"], ref["d2"], ref["nn"], o["nn"][:n], flagged)
    want = R.warp64(ref["x64"][flagged], o["nn"][:n][flagged].long(), w["tab64"])
    assert err(f"x_c {tag}", o["xc"][:n][flagged], want) < TOL.GEOM64["x_c"]
    assert (o["xc"][:n][~flagged] == F_SENT).all() and (o["nn"][:n][~flagged] == I_SENT).all()
    assert torch.equal(worklist_ids(o), torch.nonzero(flagged).reshape(-1))


def test_shading_warp_eval_small_beta(w):
    """beta = 0.1: an outlier's alpha is exactly 0, only the points within the outlier radius are kept"""
    ref = w["shd"]
    o = run_shade(w, ref["z"], 1, 0.1)
    n = o["n"]
    out, need = o["outlier"][:n], o["need"][:n]
    assert torch.equal(out.bool()[~ref["band"]], ref["out"][~ref["band"]]) and ((out == 0) | (out == 1)).all()
    assert torch.equal(need, 1 - out)
    assert (o["sdf"][:n][out == 1] == 4.0).all() and (o["sdf"][:n][out == 0] == F_SENT).all()
    check_shade_points("shade beta 0.1", w, ref, o, need == 1)


def test_shading_warp_eval_large_beta_searches_far_outliers(w):
    """beta = 1: every outlier's alpha is non-zero (asserted for these depths on the CPU), so every point is kept and the outliers --
    up to a metre from the body -- take the unbounded search (need_far).  A zero-length interval makes one outlier's alpha exactly
    0 at any beta: that point is not kept."""
    ref = w["shd"]
    dt = (ref["z"][:, 1:] - ref["z"][:, :-1]).cpu().numpy()
    assert (R.alpha4_fp32(1.0, dt) != 0).all()
    o = run_shade(w, ref["z"], 1, 1.0)
    n = o["n"]
    out = o["outlier"][:n]
    assert torch.equal(out.bool()[~ref["band"]], ref["out"][~ref["band"]])
    assert (o["need"][:n] == 1).all()
    assert (o["sdf"][:n][out == 1] == 4.0).all() and (o["sdf"][:n][out == 0] == F_SENT).all()
    every = torch.ones(n, dtype=torch.bool, device="cuda")
    check_shade_points("shade beta 1", w, ref, o, every)
    far_pts = ref["d2"].sqrt() > 0.5
    assert int(far_pts.sum()) > 1000                                          # the far branch is well populated
    check_nearest("shade beta 1, beyond 0.5 of the body", ref["x64"], w["verts"], ref["d2"], ref["nn"], o["nn"][:n], far_pts)
    # mixed: ray 5's first interval has length 0 (its first two samples coincide, a metre in front of the body)
    z = ref["z"].clone()
    z[5, 1] = z[5, 0]
    assert bool(ref["out"][5 * S]) and float(ref["d2"][5 * S].sqrt()) > 0.3
    m = run_shade(w, z, 1, 1.0)
    pid = 5 * S
    assert int(m["need"][pid]) == 0 and int(m["outlier"][pid]) == 1 and float(m["sdf"][pid]) == 4.0
    assert (m["xc"][pid] == F_SENT).all() and int(m["nn"][pid]) == I_SENT
    others = every.clone()
    others[pid] = False
    others[pid + 1] = False                                                   # (the moved sample)
    assert (m["need"][:n][others] == 1).all()
    for k in ("xc", "outlier", "sdf", "nn"):
        assert same_bits(m[k][:n][others], o[k][:n][others])
    assert torch.equal(worklist_ids(m), torch.nonzero(m["need"][:n] == 1).reshape(-1))
    assert int(m["need"][pid + 1]) == 1


def test_shading_warp_training_mode_with_and_without_bins(w):
    ref = w["shd"]
    a = run_shade(w, ref["z"], 0, 0.1)
    b = run_shade(w, ref["z"], 0, 0.1, binned=True)
    n = a["n"]
    every = torch.ones(n, dtype=torch.bool, device="cuda")
    assert (a["need"][:n] == 1).all() and (a["sdf"][:n] == F_SENT).all()
    assert torch.equal(a["outlier"][:n].bool()[~ref["band"]], ref["out"][~ref["band"]])
    check_shade_points("shade training", w, ref, a, every)
    for k in ("xc", "outlier", "need", "sdf", "nn"):
        assert same_bits(a[k], b[k]), k
    assert torch.equal(worklist_ids(a), worklist_ids(b))


def test_jacobian_on_flagged_samples(w):
    """mp_warp_jacobian with n_s = S and the shading warp's need flags: jinv of a flagged id = the 3 x 3 block of the blend table row
    of the nearest CANONICAL vertex of its x_c; with the posed neighbour as seed and without it the results are the same bits"""
    from multiply_amd import hip
    L = hip.lib()
    ref = w["shd"]
    o = run_shade(w, ref["z"], 1, 0.1)
    n = o["n"]
    flagged = o["need"][:n] == 1
    assert 0.03 * n < int(flagged.sum()) < 0.5 * n
    res = []
    for seeded in (True, False):
        jinv = torch.full((n + 16, 9), F_SENT, device="cuda")
        nn = torch.full((n + 16,), I_SENT, dtype=torch.int32, device="cuda")
        L.mp_warp_jacobian(o["xc"], o["need"], count_tensor(K), K, S, 0, w["vsorted_c"], w["cbound_c"], w["btab"], jinv, nn,
                           o["nn"] if seeded else None, w["verts_c"] if seeded else None, hip.stream())
        torch.cuda.synchronize()
        res.append((jinv, nn))
    (jinv, nn), (jinv_u, nn_u) = res
    assert same_bits(jinv, jinv_u) and torch.equal(nn, nn_u)
    assert (jinv[:n][~flagged] == F_SENT).all() and (nn[:n][~flagged] == I_SENT).all() and (jinv[n:] == F_SENT).all()
    xc = o["xc"][:n][flagged]
    d2c, nnc, gapc = R.nearest_vertex64(xc, w["verts_c"])
    nk = nn[:n][flagged]
    every = torch.ones(nk.shape[0], dtype=torch.bool, device="cuda")
    check_nearest("canonical neighbour", xc.double(), w["verts_c"], d2c, nnc, nk, every)
    assert same_bits(jinv[:n][flagged], w["btab"].reshape(V, 3, 4)[nk.long()][:, :, :3].reshape(-1, 9).contiguous())
    assert err("jinv", jinv[:n][flagged], w["tab64"][nk.long()][:, :, :3].reshape(-1, 9)) < TOL.GEOM64["jinv"]
