"""Ray setup, the box / near-body cull, the per-group fallback and the ordered compaction (csrc/rays.hip) through the C ABI against
the float64 reference (oracle/geom_oracle64.py).  Scene and the conditions it meets: tests/geom_scene.py,
tests/test_geom_oracle64_cpu.py.  Every set / index / count assertion is exact; dirs and far are bounded by tolerances.GEOM64."""
import pytest
import torch

from oracle import geom_oracle64 as R
from tests import geom_scene as G
from tests import tolerances as TOL

pytestmark = pytest.mark.gpu

GRAZE = 1e-4          # rays whose float64 margin to the box is below this may fall on either side (the hull test's bound)


@pytest.fixture(scope="module")
def sc(smpl_tables):
    return G.device_scene(smpl_tables)


def err(name, got, want):
    e = (got.double().cpu() - want.double().cpu()).abs().max().item() if got.numel() else 0.0
    print(f"[geom64] {name}: max abs err {e:.3e}")
    return e


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ray_setup_matches_float64(sc, n):
    """skewed intrinsics, a rotated camera inside the bounding sphere (radius 3) and the same camera outside a sphere of radius 1,
    where the rays towards the rim miss it: far = 0 there, never NaN"""
    uv = sc["uv"][1000:1000 + n]
    dirs, far = G.ray_setup(uv, sc["K"], sc["pose"], G.RADIUS)
    d64, c64 = R.camera_rays64(uv, sc["K"], sc["pose"])
    f64, under = R.sphere_far64(c64, d64, G.RADIUS)
    assert err(f"dirs[{n}]", dirs, d64) < TOL.GEOM64["dirs"] and err(f"far[{n}]", far, f64) < TOL.GEOM64["far"]
    uvo = G.outside_camera_pixels()[:n]
    dirs, far = G.ray_setup(uvo, sc["K"], sc["pose"], 1.0)
    d64, c64 = R.camera_rays64(uvo, sc["K"], sc["pose"])
    f64, under = R.sphere_far64(c64, d64, 1.0)
    far, under = far.cpu(), under.cpu()
    assert not far.isnan().any() and (far >= 0).all()
    miss, hit = under < -G.FAR_GRAZE, under > G.FAR_GRAZE
    assert int(miss.sum()) > 0 and (far[miss] == 0).all()
    assert err(f"dirs outside[{n}]", dirs, d64) < TOL.GEOM64["dirs"]
    assert err(f"far outside[{n}]", far[hit], f64[hit]) < TOL.GEOM64["far"] and (far[hit] > 0).all()


def _flags64(sc, obb, dirs=None):
    d = sc["dirs"] if dirs is None else dirs
    hit, margin = R.ray_box64(sc["cam"], d, obb.cuda()[:15])
    return hit.cpu(), margin.cpu()


def _expected(got_inv, want, margin, n, group):
    """the reference's hit set for the first n rays; a ray that grazes the box takes the side the kernel gave it"""
    graze = margin[:n].abs() < GRAZE
    f = torch.where(graze, got_inv[:n] >= 0, want[:n])
    return R.compact(R.group_fallback(f, group)), int(graze.sum())


def _check(tag, got, want_compact, n):
    hit, count, inv = got
    w_hit, w_inv, w_n = want_compact
    assert count == w_n, f"{tag}: hit_count {count}, reference {w_n}"
    assert torch.equal(hit[:count], w_hit), f"{tag}: hit_index"
    assert (hit[1:count] > hit[:count - 1]).all(), f"{tag}: hit_index not strictly ascending"
    assert (hit[count:] == G.SENTINEL).all(), f"{tag}: hit_index written behind the count"
    assert torch.equal(inv[:n], w_inv), f"{tag}: inv_index"
    assert torch.equal(inv[hit[:count]], torch.arange(count)), f"{tag}: inv_index[hit_index[i]] != i"
    assert (inv[n:] == G.SENTINEL).all(), f"{tag}: inv_index written behind the last ray"


def test_box_flags_match_float64(sc):
    """the device's PCA box, and two hand-made axis-aligned boxes with rays exactly parallel to their faces (the |dd| < 1e-12 branch:
    inside the slab pair for the body box, outside it for the box round the body's top)"""
    n = G.R_FULL
    verts = sc["verts"].cpu().numpy()
    pd = G.parallel_dirs(sc["dirs"].cpu()).cuda()
    assert int((pd == 0).any(1).sum()) > 500
    for name, obb, dirs in (("pca", sc["obb"], None), ("axis body", G.axis_box(verts), pd), ("axis top", G.axis_box(verts, "top"), pd)):
        want, margin = _flags64(sc, obb, dirs)
        got = G.ray_cull(sc, obb, n, 0, dirs=dirs)
        n_graze = int((margin.abs() < GRAZE).sum())
        diff = (got[2][:n] >= 0) != want
        print(f"[geom64] {name} box: {int(want.sum())} of {n} rays hit, {n_graze} graze, {int(diff.sum())} flags differ")
        assert 0 < int(want.sum()) < n and n_graze <= 0.005 * n               # the condition, by the reference alone
        assert (margin[diff].abs() < GRAZE).all(), (name, margin[diff][:5])
        exp, _ = _expected(got[2], want, margin, n, 0)
        _check(name, got, exp, n)


@pytest.mark.parametrize("n", [1, 63, 64, 1023, 1024, 1025, 2048, G.R_FULL])
def test_compaction_is_ordered_and_exact(sc, n):
    """the three-kernel scan and scatter at its wave and block boundaries, with boxes that select every ray, none (the single group's
    fallback then gives ray 0) and a mixed set"""
    cases = (("everything", G.everything_box()), ("nothing", G.nothing_box()), ("mixed", sc["obb"]),
             ("spot", G.spot_box(sc["cam"].cpu(), sc["dirs"].cpu())))
    for name, obb in cases:
        want, margin = _flags64(sc, obb)
        got = G.ray_cull(sc, obb, n, 0)
        exp, n_graze = _expected(got[2], want, margin, n, 0)
        _check(f"{name}[{n}]", got, exp, n)
        if name == "everything":
            assert got[1] == n and n_graze == 0
        if name == "nothing":
            assert got[1] == 1 and got[0][0] == 0 and n_graze == 0
    if n == G.R_FULL:
        assert 0.3 * n < G.ray_cull(sc, sc["obb"], n, 0)[1] < 0.9 * n           # "mixed" is mixed


@pytest.mark.parametrize("group", [0, 1, 96, 1024, 1500])
def test_group_fallback(sc, group):
    """whole convergence groups miss the spot box -- the last, partial one among them: each contributes exactly its first ray, a
    group with a hit nothing extra"""
    n = G.R_FULL
    for name, obb in (("spot", G.spot_box(sc["cam"].cpu(), sc["dirs"].cpu())), ("nothing", G.nothing_box()), ("mixed", sc["obb"])):
        want, margin = _flags64(sc, obb)
        got = G.ray_cull(sc, obb, n, group)
        exp, n_graze = _expected(got[2], want, margin, n, group)
        _check(f"{name} group {group}", got, exp, n)
        if name == "spot":
            assert n_graze == 0
            gs = group or n
            firsts = [g0 for g0 in range(0, n, gs) if not bool(want[g0:g0 + gs].any())]
            extra = sorted(set(got[0][:got[1]].tolist()) - set(torch.nonzero(want).reshape(-1).tolist()))
            assert extra == firsts
            if group > 1:
                assert firsts and firsts[-1] == (n // gs) * gs and n % gs != 0          # the partial last group is one of them
        if name == "nothing":
            assert got[0][:got[1]].tolist() == list(range(0, n, group or n))


@pytest.mark.parametrize("group", [0, 96])
def test_near_cull_drops_only_rays_clear_of_the_body(sc, group):
    n = G.R_FULL
    box = G.ray_cull(sc, sc["obb"], n, group)
    near = G.ray_cull(sc, sc["obb"], n, group, near_beta=0.1)
    kept_box, kept_near = box[2][:n] >= 0, near[2][:n] >= 0
    fallback = torch.zeros(n, dtype=torch.bool)
    if group:
        fallback[::group] = True
    dist = R.segment_vertex_distance64(sc["cam"], sc["dirs"], G.NEAR, sc["far"], sc["verts"]).cpu()
    dropped = kept_box & ~kept_near & ~fallback
    print(f"[geom64] near cull (group {group}): {int(kept_box.sum())} rays pass the box, {int(dropped.sum())} dropped; nearest dropped "
          f"ray {float(dist[dropped].min()) if dropped.any() else float('nan'):.4f} from a vertex; "
          f"{int((kept_near & (dist > 0.12)).sum())} kept beyond 0.12")
    assert (dist[dropped] > 0.1).all()                                        # (a) strict: reach = radius + 0.1005
    assert int(dropped.sum()) > 0                                             # (b)
    assert int((kept_box & (dist > 0.12)).sum()) >= 0.05 * int(kept_box.sum())   # its condition, by the reference alone
    assert not (kept_near & ~kept_box & ~fallback).any()                      # (c)
    # the survivors are compacted like any flag set; a group's first ray that did not pass the box is there only as the fallback of
    # a group the cull emptied
    _check(f"near group {group}", near, R.compact(kept_near), n)
    for g0 in torch.nonzero(kept_near & ~kept_box).reshape(-1).tolist():
        assert group and int(kept_near[g0:g0 + group].sum()) == 1


def test_near_cull_keeps_every_ray_whose_outliers_still_weigh(sc):
    """(d) beta = 1: alpha(4, beta, far - near) != 0 for every ray (asserted for the scene on the CPU): bit for bit mp_ray_cull"""
    n = G.R_FULL
    assert (R.alpha4_fp32(1.0, (sc["far"].cpu() - G.NEAR).numpy()) != 0).all()
    for group in (0, 96):
        box = G.ray_cull(sc, sc["obb"], n, group)
        near = G.ray_cull(sc, sc["obb"], n, group, near_beta=1.0)
        assert box[1] == near[1] and torch.equal(box[0], near[0]) and torch.equal(box[2], near[2])


def test_near_cull_rejects_missing_tables(sc):
    """(e) NULL cbound, far or beta: status -1 from the wrapper, nothing launched"""
    from multiply_amd import hip
    n = 300
    i32 = dict(dtype=torch.int32, device="cuda")
    beta = torch.tensor([0.1], device="cuda")
    for cbound, far, b in ((None, sc["far"], beta), (sc["cbound"], None, beta), (sc["cbound"], sc["far"], None)):
        hit, inv, count = torch.full((n,), G.SENTINEL, **i32), torch.full((n,), G.SENTINEL, **i32), torch.full((1,), G.SENTINEL, **i32)
        scan_tmp = torch.full((n + 9,), G.SENTINEL, **i32)
        with pytest.raises(RuntimeError, match="code -1"):
            hip.lib().mp_ray_cull_near(sc["dirs"], sc["pose_d"], sc["obb"], cbound, far, b, G.NEAR, n, 0, hit, count, inv, scan_tmp,
                                       hip.stream())
        torch.cuda.synchronize()
        for t in (hit, inv, count, scan_tmp):
            assert (t == G.SENTINEL).all()


@pytest.mark.parametrize("n_hit", [1, 300, G.R_FULL])
def test_hits_from_index(n_hit):
    from multiply_amd import hip
    n = G.R_FULL
    g = torch.Generator().manual_seed(n_hit)
    ids = torch.sort(torch.randperm(n, generator=g)[:n_hit]).values
    i32 = dict(dtype=torch.int32, device="cuda")
    hit = torch.full((n + 8,), G.SENTINEL, **i32)
    hit[:n_hit] = ids.to(torch.int32).cuda()
    inv, count = torch.full((n + 8,), G.SENTINEL, **i32), torch.full((2,), G.SENTINEL, **i32)
    hip.lib().mp_ray_hits_from_index(hit, n_hit, n, count, inv, hip.stream())
    torch.cuda.synchronize()
    want = torch.full((n,), -1, dtype=torch.int64)
    want[ids] = torch.arange(n_hit)
    assert count.tolist() == [n_hit, G.SENTINEL]
    assert torch.equal(inv[:n].cpu().long(), want) and (inv[n:] == G.SENTINEL).all()
    assert torch.equal(hit[:n_hit].cpu().long(), ids) and (hit[n_hit:] == G.SENTINEL).all()
