"""The float64 geometry reference (oracle/geom_oracle64.py) pinned to what the repository already trusts -- the fp32 oracle, the
reference's golden rays, oracle/obb_oracle.py -- and the conditions the GPU tests of the geometry front end rely on
(tests/test_rays_gpu.py, tests/test_warp_samples_gpu.py), asserted on the shared scene (tests/geom_scene.py) by the reference alone."""
import numpy as np
import pytest
import torch

from oracle import geom_oracle64 as R
from oracle import multiply_oracle as O
from oracle.obb_oracle import rays_hitting_box
from tests import geom_scene as G
from tests import tolerances as TOL
from tests.util import t32


def err(name, got, want):
    e = (torch.as_tensor(got).double() - torch.as_tensor(want).double()).abs().max().item()
    print(f"[oracle64] {name}: max abs err {e:.3e}")
    return e


@pytest.fixture(scope="module")
def scene(smpl_tables):
    prm = G.body_params()
    so = O.SMPLServerOracle(smpl_tables, prm[76:].numpy())
    body = so.forward(prm[0], prm[1:4], prm[4:76], prm[76:])
    K, pose = G.camera()
    uv = G.pixels()
    dirs, cam = O.get_camera_rays(uv, pose, K)
    verts = body["smpl_verts"]
    box = G.pca_box(verts.numpy())
    hit, margin = R.ray_box64(cam, dirs, box)
    far = O.sphere_far(cam[None].expand(uv.shape[0], -1), dirs, G.RADIUS)[:, 0]
    return dict(so=so, verts=verts, tfs=body["smpl_tfs"], K=K, pose=pose, uv=uv, dirs=dirs, cam=cam, box=box, hit=hit, margin=margin,
                far=far)


def test_camera_rays_and_far_root(scene, golden):
    uv, pose, K = t32(golden["g1_uv"])[0], t32(golden["g1_pose"])[0], t32(golden["g1_K"])[0]
    d64, c64 = R.camera_rays64(uv, K, pose)
    d32, c32 = O.get_camera_rays(uv, pose, K)
    assert err("golden dirs", d64, golden["g1_dirs"][0]) < 5e-7 and err("dirs vs fp32 oracle", d64, d32) < 0.5 * TOL.GEOM64["dirs"]
    assert torch.equal(c64.float(), c32)
    far64, under = R.sphere_far64(c64, d64, 3.0)
    assert err("far vs fp32 oracle", far64, O.sphere_far(c32[None].expand(uv.shape[0], -1), d32, 3.0)[:, 0]) < 0.5 * TOL.GEOM64["far"]
    # the scene's skewed camera
    d64, c64 = R.camera_rays64(scene["uv"], scene["K"], scene["pose"])
    assert err("scene dirs vs fp32 oracle", d64, scene["dirs"]) < 0.5 * TOL.GEOM64["dirs"]
    assert (d64.norm(dim=1) - 1).abs().max() < 1e-15
    far64, under = R.sphere_far64(c64, d64, G.RADIUS)
    assert (under > 1.0).all() and err("scene far vs fp32 oracle", far64, scene["far"]) < 0.5 * TOL.GEOM64["far"]
    # the camera outside a sphere of radius 1: hits and misses among any prefix the GPU test runs, few rays near the tangent
    uvo = G.outside_camera_pixels()
    d64, c64 = R.camera_rays64(uvo, scene["K"], scene["pose"])
    far64, under = R.sphere_far64(c64, d64, 1.0)
    assert c64.norm() > 1.0 and not far64.isnan().any()
    assert (far64[under < 0] == 0).all() and (far64[under > 0] > 0).all()
    for n in (255, 256, 257):
        assert int((under[:n] < -G.FAR_GRAZE).sum()) > 20 and int((under[:n] > G.FAR_GRAZE).sum()) > 20
    assert under[0] < -G.FAR_GRAZE                                            # the one-ray launch is a miss
    assert int((under.abs() < G.FAR_GRAZE).sum()) <= 0.05 * uvo.shape[0]


def test_ray_box_matches_the_published_slab_test(scene):
    cam, dirs, verts = scene["cam"], scene["dirs"], scene["verts"].numpy()
    cases = [("pca", dirs, scene["box"]), ("axis body", G.parallel_dirs(dirs), G.axis_box(verts)),
             ("axis top", G.parallel_dirs(dirs), G.axis_box(verts, "top")), ("spot", dirs, G.spot_box(cam, dirs))]
    for name, d, box in cases:
        b = box.double().numpy()
        want, wm = rays_hitting_box(cam.numpy(), d.numpy(), b[0:3], b[3:12].reshape(3, 3), b[12:15])
        hit, margin = R.ray_box64(cam, d, box)
        assert torch.equal(torch.nonzero(hit).reshape(-1), torch.from_numpy(want)), name
        fin = np.isfinite(wm)
        assert np.array_equal(fin, torch.isfinite(margin).numpy()) and np.allclose(margin.numpy()[fin], wm[fin], rtol=1e-12, atol=1e-12)
        n_graze = int((margin.abs() < 1e-4).sum())
        print(f"[oracle64] {name} box: {int(hit.sum())} of {d.shape[0]} rays hit, {n_graze} within 1e-4 of an edge")
        assert 0 < int(hit.sum()) < d.shape[0]
        assert n_graze <= 0.005 * d.shape[0]                                   # the share the GPU test leaves out
    # the parallel branch: rays with a component exactly 0, and both of its outcomes (inside / outside the slab pair)
    pd = G.parallel_dirs(dirs)
    par = (pd == 0).any(1)
    assert int(par.sum()) > 500
    body_hit, _ = R.ray_box64(cam, pd, G.axis_box(verts))
    top_hit, _ = R.ray_box64(cam, pd, G.axis_box(verts, "top"))
    assert bool(body_hit[par].any()) and bool((~top_hit[par]).any())
    top = G.axis_box(verts, "top").double()
    o = (cam.double() - top[0:3]).abs()
    assert bool((o[:2] > top[12:14]).any())                                    # the camera is outside one slab pair of the top box


def test_group_fallback_and_compaction_by_hand(scene):
    f = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0], dtype=torch.bool)
    assert R.group_fallback(f, 0).tolist() == f.tolist()
    assert R.group_fallback(f, 3).tolist() == [0, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0]          # groups 3-5 and 9-10 (partial) had no hit
    assert R.group_fallback(f, 1).all()
    assert R.group_fallback(torch.zeros(5, dtype=torch.bool), 0).tolist() == [1, 0, 0, 0, 0]
    hit, inv, n = R.compact(R.group_fallback(f, 3))
    assert hit.tolist() == [2, 3, 8, 9] and n == 4 and inv.tolist() == [-1, -1, 0, 1, -1, -1, -1, -1, 2, 3, -1]
    # the spot box of the GPU test: some group is hit, whole groups (the last, partial one among them) miss
    cam, dirs = scene["cam"], scene["dirs"]
    spot, _ = R.ray_box64(cam, dirs, G.spot_box(cam, dirs))
    for gs in (96, 1024, 1500):
        assert G.R_FULL % gs != 0
        groups = [bool(spot[g0:g0 + gs].any()) for g0 in range(0, G.R_FULL, gs)]
        assert any(groups) and not all(groups) and not groups[-1], (gs, groups)
        extra = R.group_fallback(spot, gs) & ~spot
        assert torch.nonzero(extra).reshape(-1).tolist() == [g * gs for g, h in enumerate(groups) if not h]
    nothing, _ = R.ray_box64(cam, dirs, G.nothing_box())
    everything, _ = R.ray_box64(cam, dirs, G.everything_box())
    assert not nothing.any() and everything.all()


def test_near_cull_conditions(scene):
    cam, dirs, far, hit = scene["cam"], scene["dirs"], scene["far"], scene["hit"]
    dist = R.segment_vertex_distance64(cam, dirs, G.NEAR, far, scene["verts"])
    # against a direct statement on a few rays: dense points of the segment
    for r in (0, 1500, 3000):
        t = torch.linspace(G.NEAR, float(far[r]), 20001, dtype=torch.float64)
        p = cam.double()[None] + t[:, None] * dirs[r].double()[None]
        dense = torch.cdist(p, scene["verts"].double()).min()
        assert 0 <= dense - dist[r] < 1e-4
    clear = hit & (dist > 0.12)
    print(f"[oracle64] {int(hit.sum())} rays pass the box, {int(clear.sum())} of them stay farther than 0.12 from every vertex")
    assert int(clear.sum()) >= 0.05 * int(hit.sum())
    assert int((hit & (dist < 0.08)).sum()) >= 0.2 * int(hit.sum())           # and many rays do come near the body
    dt = (far - G.NEAR).numpy()
    assert (R.alpha4_fp32(1.0, dt) != 0).all()                                # beta = 1: the near cull must keep every ray
    assert (R.alpha4_fp32(0.1, dt) == 0).all()                                # beta = 0.1: it may drop the clear ones


def test_alpha4_is_the_fp32_statement():
    dt = np.array([0.0, 1e-6, 1e-3, 0.03, 5.0], dtype=np.float32)
    a = R.alpha4_fp32(1.0, dt)
    want = 1.0 - np.exp(-(0.5 * np.exp(-4.0)) * dt.astype(np.float64))
    assert a.dtype == np.float32 and a[0] == 0 and np.allclose(a, want, rtol=1e-4, atol=1.2e-7)   # 2 ulp of 1
    assert (R.alpha4_fp32(0.1, dt) == 0).all() and (R.alpha4_fp32(0.2, dt) == 0).all()   # expm1(-4 / beta) rounds to -1


def _warp_inputs(scene, every=1):
    ids = G.pick_rays(torch.nonzero(scene["hit"]).reshape(-1))[::every]
    return ids, scene["dirs"][ids]


def test_nearest_vertex_and_warp_match_the_fp32_oracle(scene):
    so, verts, tfs = scene["so"], scene["verts"], scene["tfs"]
    ids, d = _warp_inputs(scene, every=4)                                     # 175 of the 700 rays: the CPU brute force stays quick
    z = G.sampler_depths()[::4]
    x64 = G.sample_points(scene["cam"], d, z, G.NS)
    x32 = x64.float()
    d2, nn, gap = R.nearest_vertex64(x32, verts)
    d2_32, nn_32 = O.knn1(x32, verts)
    same = nn == nn_32
    band = (d2.sqrt() - 0.1).abs() < 1e-6
    print(f"[oracle64] {x32.shape[0]} points: {int((~same).sum())} fp32 argmins differ, {int(band.sum())} on the outlier radius, "
          f"{int(R.outlier64(d2).sum())} outliers")
    assert int(same.sum()) >= 0.999 * x32.shape[0] and int(band.sum()) <= 0.001 * x32.shape[0]
    # where the fp32 search took another vertex, that vertex is as near within the fp32 evaluation error
    other = ((x32.double() - verts.double()[nn_32]) ** 2).sum(-1)
    assert (other - d2 <= G.d2_eval_bound(d2)).all()
    assert 0.03 * x32.shape[0] < int((~R.outlier64(d2)).sum()) < 0.5 * x32.shape[0]     # both kinds are well populated
    xc_w, out_w = O.deform_inverse(x32, tfs, verts, so.weights)
    assert torch.equal(out_w[~band], R.outlier64(d2)[~band])
    tab = R.blend_table64(so.weights, tfs)
    xc = R.warp64(x32, nn, tab)
    assert err("x_c vs fp32 oracle", xc[same], xc_w[same]) < 0.5 * TOL.GEOM64["x_c"]
    w_c, _, idx_c = O.query_weights(xc_w, so.verts_c, so.weights)
    d2c, nnc, gapc = R.nearest_vertex64(xc_w, so.verts_c)
    assert int((nnc == idx_c).sum()) >= 0.999 * x32.shape[0]
    # ties resolve to the lowest id
    v = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0.0, 2, 0]])
    d2t, nnt, gapt = R.nearest_vertex64(torch.tensor([[1.0, 0.5, 0], [0.5, 0, 0]]), v)
    assert nnt.tolist() == [1, 0] and gapt.tolist() == [0.0, 0.0] and d2t.tolist() == [0.25, 0.25]


def test_blend_table_matches_the_library_inverse(scene):
    so, tfs = scene["so"], scene["tfs"]
    tab = R.blend_table64(so.weights, tfs)
    T = torch.einsum("vj,jab->vab", so.weights.double(), tfs.double())
    assert tab.shape == (6890, 3, 4)
    assert err("I vs torch.linalg.inv", tab[:, :, :3], torch.linalg.inv(T[:, :3, :3])) < 1e-12
    assert err("c", tab[:, :, 3], T[:, :3, 3] / T[:, 3, 3:4]) < 1e-15
    # the fp32 oracle's own distance to float64 on the same inputs (quoted in tolerances.GEOM64)
    T32 = torch.einsum("vj,jab->vab", so.weights, tfs)
    e_i = err("fp32 oracle I vs float64", T32[:, :3, :3].inverse(), tab[:, :, :3])
    e_c = err("fp32 oracle c vs float64", T32[:, :3, 3] / T32[:, 3, 3:4], tab[:, :, 3])
    assert max(e_i, e_c) < 0.5 * TOL.GEOM64["blend_table"] and e_i < 0.5 * TOL.GEOM64["jinv"]
    x = torch.randn(6890, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    full = torch.einsum("vab,vb->va", torch.linalg.inv(T), torch.cat([x, torch.ones(6890, 1, dtype=torch.float64)], 1))[:, :3]
    assert err("warp64 vs the 4x4 inverse", R.warp64(x, torch.arange(6890), tab), full) < 1e-12


def test_shading_depths_keep_every_outlier_weighted_at_beta_one(scene):
    z = G.shade_depths()
    dt = (z[:, 1:] - z[:, :-1]).numpy()
    assert z.shape == (G.K_WARP, G.S_SHADE + 1) and (dt > 1e-3).all()
    a = R.alpha4_fp32(1.0, dt)
    assert (a != 0).all() and (a > 1e-6).all()                               # far from the rounding threshold of 1 - exp(-x)
    assert (R.alpha4_fp32(0.1, dt) == 0).all()
    assert R.alpha4_fp32(1.0, np.zeros(3, np.float32)).tolist() == [0.0, 0.0, 0.0]     # a zero-length interval: exactly 0 at any beta
    zs = G.sampler_depths()
    assert zs.shape == (G.K_WARP, G.ZSTRIDE) and zs[:, G.NS:].isnan().all() and (zs[:, 1:G.NS] > zs[:, :G.NS - 1]).all()
    # the first sample of every ray is far from the body (the zero-interval case of the GPU test sits there)
    ids, d = _warp_inputs(scene)
    x0 = G.sample_points(scene["cam"], d, z, 1)
    d2, _, _ = R.nearest_vertex64(x0, scene["verts"])
    assert (d2.sqrt() > 0.3).all()
