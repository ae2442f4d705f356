"""Face index of the mesh signed distance (csrc/mesh_index.hip): mp_mesh_index_signed_distance returns the bits of the brute-force
mp_mesh_signed_distance -- on ordinary, degenerate and non-finite inputs --, follows a mesh that changes, and every caller
(training flags, the fit's target distances, the interpenetration term) computes the same under 'index' and 'brute'."""
import numpy as np
import pytest
import torch

from oracle import multiply_oracle as O

pytestmark = pytest.mark.gpu


def icosphere(n=3, radius=0.5, base=8):
    """test_mesh_flags_gpu's recipe: an octahedron subdivided n times (8 * 4^n faces: 512, 8 192 -- powers of two); base=20 starts
    from the icosahedron instead (20 * 4^n faces: 1 280, 20 480 -- the leaf count is no power of two, the tree has empty leaves)"""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    if base == 20:
        t = (1 + 5 ** 0.5) / 2
        v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                      [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float) / (1 + t * t) ** 0.5
        f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                      [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                      [9, 8, 1]])
    for _ in range(n):
        cache, vs, nf = {}, list(v), []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (vs[a] + vs[b]) / 2
                cache[k] = len(vs)
                vs.append(m / np.linalg.norm(m))
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v, f = np.array(vs), np.array(nf)
    return torch.tensor(v * radius, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def squashed(n, radius=0.5, base=20):
    """the squashed, offset sphere of test_mesh_flags_gpu: not symmetric, not centred"""
    v, f = icosphere(n, radius, base)
    return v * torch.tensor([1.0, 1.4, 0.7]) + torch.tensor([0.03, -0.02, 0.05]), f


N_S = 17        # samples per ray of the flag checks


def point_sets(v, f, seed):
    """{name: (n,3)} around the mesh (v, f): ~6 000 points in all"""
    g = torch.Generator().manual_seed(seed)
    fv = v[f]
    lo, hi = v.min(0).values, v.max(0).values
    ctr, ext = (lo + hi) / 2, (hi - lo).max()
    pick = lambda t, k: t[torch.randperm(t.shape[0], generator=g)[:k]]
    sets = {}
    mix = (torch.rand(150 * N_S, 3, generator=g) - 0.5) * 2.0                 # the existing test's mix: inside, near, far
    mix[:N_S * 20] *= 0.2
    mix[N_S * 20:N_S * 40] = mix[N_S * 20:N_S * 40] * 0.1 + torch.tensor([0.9, 0.9, 0.9])
    sets["mix"] = mix * (ext / 1.4) + ctr
    near = pick(fv.mean(1), 600)
    sets["near"] = near + 2e-3 * ext * torch.randn(near.shape, generator=g)
    d = torch.randn(300, 3, generator=g)
    sets["far"] = ctr + 10.0 * ext * d / d.norm(dim=1, keepdim=True)
    sets["on vertices"] = pick(v, 400)
    e = pick(torch.cat([fv[:, [0, 1]], fv[:, [1, 2]], fv[:, [2, 0]]]), 400)
    sets["on edge midpoints"] = (e[:, 0] + e[:, 1]) / 2
    sets["on centroids"] = pick(fv.mean(1), 400)
    p = (torch.rand(600, 3, generator=g) - 0.5) * 1.6 * ext + ctr
    p[:, 1] = pick(v, 600)[torch.arange(600) % min(600, v.shape[0]), 1]          # y of a vertex, bit for bit: the half-open rule
    sets["vertex y"] = p
    p = (torch.rand(600, 3, generator=g) - 0.5) * 1.6 * ext + ctr
    p[:, 1:] = pick(v, 600)[torch.arange(600) % min(600, v.shape[0]), 1:]        # the ray runs through a vertex
    sets["vertex y and z"] = p
    return sets


def brute(pts, fv):
    from multiply_amd import hip
    sd = torch.empty(pts.shape[0], device="cuda")
    hip.lib().mp_mesh_signed_distance(pts, pts.shape[0], fv, fv.shape[0], sd, hip.stream())
    return sd


def indexed(pts, fv):
    """the C entry points one by one, as hip.MeshIndex drives them"""
    from multiply_amd import hip
    L, F = hip.lib(), fv.shape[0]
    buf = torch.empty(int(L.mp_mesh_index_bytes(F)), dtype=torch.uint8, device="cuda")
    keys = torch.empty(F, dtype=torch.int32, device="cuda")
    L.mp_mesh_index_keys(fv, F, buf, keys, hip.stream())
    L.mp_mesh_index_build(fv, F, torch.sort(keys, stable=True).indices, buf, hip.stream())
    sd = torch.empty(pts.shape[0], device="cuda")
    L.mp_mesh_index_signed_distance(pts, pts.shape[0], buf, F, sd, None, hip.stream())
    return sd


def bits_equal(a, b):
    """torch.equal, signs of zeros and NaNs included"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_index_equals_brute(pts, fv, what):
    pts, fv = pts.float().cuda().contiguous(), fv.float().reshape(-1, 9).cuda().contiguous()
    want, got = brute(pts, fv), indexed(pts, fv)
    torch.cuda.synchronize()
    bad = (want.view(torch.int32) != got.view(torch.int32)).nonzero().flatten()
    print(f"[index = brute] {what}: {pts.shape[0]} points x {fv.shape[0]} faces, inside {(want < 0).float().mean().item():.3f}, "
          f"{bad.numel()} differ" + (f"; first: point {pts[bad[0]].tolist()} brute {want[bad[0]].item()!r} index {got[bad[0]].item()!r}"
                                     if bad.numel() else ""))
    assert torch.equal(want, got), what
    assert bad.numel() == 0, what              # the signs of zeros (points on the surface) too
    return want


@pytest.fixture(scope="module")
def sphere3():
    v, f = squashed(3)
    return v, f, point_sets(v, f, 0)


@pytest.mark.parametrize("level,base,faces", [(3, 20, 1280), (5, 20, 20480), (3, 8, 512), (5, 8, 8192)])
def test_index_equals_brute_force_on_spheres(level, base, faces, sphere3):
    """1 280 and 20 480 faces (160 and 2 560 leaves: trees padded with empty leaves, the larger one 13 levels deep), and the recipe
    of test_mesh_flags_gpu as it stands (512 and 8 192 faces: full trees)"""
    v, f, sets = sphere3 if (level, base) == (3, 20) else (*squashed(level, base=base), None)
    sets = point_sets(v, f, level + base) if sets is None else sets
    assert f.shape[0] == faces
    n = 0
    for name, pts in sets.items():
        assert_index_equals_brute(pts, v[f], f"sphere of {faces} faces, {name}")
        n += pts.shape[0]
    assert 5500 <= n <= 6500


def test_index_equals_brute_force_on_translated_mesh(sphere3):
    """coordinates of magnitude 50: the rounding of p - q in tri_dist2 is 100 times that of the unit-sized mesh"""
    v, f, sets = sphere3
    t = torch.tensor([50.0, -50.0, 50.0])
    vt = v + t
    for name, pts in sets.items():
        assert_index_equals_brute(pts + t, vt[f], f"translated icosphere(3), {name}")


@pytest.mark.parametrize("F", [1, 7, 9])
def test_index_equals_brute_force_on_tiny_trees(F):
    v, f = squashed(1, base=8)
    g = torch.Generator().manual_seed(F)
    fv = v[f][torch.randperm(f.shape[0], generator=g)[:F]]                    # F = 9: one full leaf and one face
    pts = torch.cat([(torch.rand(500, 3, generator=g) - 0.5) * 2.0, fv.reshape(-1, 3), fv.mean(1)])
    assert_index_equals_brute(pts, fv, f"{F} faces")
    if F == 1:
        # one triangle that contains the ray's direction (its normal has no x component) is never crossed: every sign positive
        tri = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 1.0, 0.5]]])
        sd = assert_index_equals_brute(torch.cat([pts, tri.reshape(-1, 3), tri.mean(1)]), tri, "1 face along the ray")
        assert bool((sd >= 0).all()) and not bool(torch.signbit(sd).any())


def test_index_equals_brute_force_on_degenerate_meshes(sphere3):
    g = torch.Generator().manual_seed(3)
    # planar: a triangulated grid in the plane z = 0.25 (zero extent in z: in the keys' scale and in every box)
    k = 12
    xy = torch.stack(torch.meshgrid(torch.linspace(-0.5, 0.5, k), torch.linspace(-0.4, 0.6, k), indexing="ij"), -1).reshape(-1, 2)
    vp = torch.cat([xy, torch.full((k * k, 1), 0.25)], 1)
    q = torch.tensor([[i * k + j, (i + 1) * k + j, i * k + j + 1] for i in range(k - 1) for j in range(k - 1)] +
                     [[(i + 1) * k + j, (i + 1) * k + j + 1, i * k + j + 1] for i in range(k - 1) for j in range(k - 1)])
    pts = torch.cat([(torch.rand(1500, 3, generator=g) - 0.5) * 1.6, vp,
                     torch.cat([(torch.rand(500, 2, generator=g) - 0.5) * 1.2, torch.full((500, 1), 0.25)], 1)])    # in the plane too
    assert_index_equals_brute(pts, vp[q], "planar mesh")
    # duplicated faces (every crossing counted twice) and a zero-area face
    v, f, sets = sphere3
    fv = v[f]
    dup = torch.cat([fv[:200], fv, fv[100:300], fv[5:6, [0, 0, 0]], fv[7:8, [0, 1, 1]]])
    assert_index_equals_brute(torch.cat([sets["mix"], sets["on vertices"], sets["vertex y"]]), dup, "duplicated + zero-area faces")


def test_index_equals_brute_force_on_nested_and_disjoint_surfaces(sphere3):
    v, f, sets = sphere3
    fv = v[f]
    shift = torch.tensor([1.3, 0.1, -0.2])
    both = torch.cat([fv, fv + shift])
    pts = torch.cat([sets["mix"], sets["mix"] + shift, sets["vertex y"], sets["on vertices"] + shift])
    assert_index_equals_brute(pts, both, "two disjoint spheres")
    ctr = (v.min(0).values + v.max(0).values) / 2
    inner = (fv - ctr) * 0.4 + ctr
    sd = assert_index_equals_brute(torch.cat([sets["mix"], ctr[None]]), torch.cat([fv, inner]), "nested spheres")
    assert sd[-1].item() > 0, "parity: inside the inner sphere counts as outside"


def test_non_finite_points_get_what_brute_force_gives_and_disturb_nobody(sphere3):
    v, f, sets = sphere3
    pts = sets["mix"][:640].clone()
    clean = assert_index_equals_brute(pts, v[f], "finite points")
    inf, nan = float("inf"), float("nan")
    odd = {3: [nan, 0.1, 0.2], 70: [0.1, nan, nan], 131: [inf, 0.0, 0.1], 200: [-inf, 0.0, 0.1], 333: [0.1, inf, 0.0],
           400: [0.0, 0.1, -inf], 500: [inf, -inf, inf]}
    for i, p in odd.items():
        pts[i] = torch.tensor(p)
    got = assert_index_equals_brute(pts, v[f], "with NaN and +-inf points")
    keep = torch.ones(pts.shape[0], dtype=torch.bool)
    keep[list(odd)] = False
    assert torch.equal(got[keep.cuda()], clean[keep.cuda()])


def test_index_matches_float64_oracle(sphere3):
    """|sdist| of EVERY point against float64 at 1e-5.  Signs and flags on every set but the rays THROUGH a vertex ("vertex y and
    z", the last set): there an edge's zc equals p.z up to the rounding of u.z + (w.z - u.z), so fp32 (brute force and index
    alike, see the equality tests) and float64 may count that edge differently -- the rule has no right answer on such a ray.
    The number of such rays on which the sign differs is printed."""
    from multiply_amd import hip
    v, f, sets = sphere3
    fv = v[f].contiguous()
    assert list(sets)[-1] == "vertex y and z"
    through = sets["vertex y and z"]
    want_t = O.mesh_signed_distance(through, fv).reshape(-1)
    got_t = indexed(through.cuda().contiguous(), fv.reshape(-1, 9).cuda()).cpu().double()
    err_t = (got_t.abs() - want_t.abs()).abs()
    flips = int(((got_t < 0) != (want_t < 0)).sum())
    print(f"[parity] rays through a vertex: | |sd| - |sd64| | max {err_t.max().item():.3e}; sign differs on {flips} of {through.shape[0]}")
    assert err_t.max() < 1e-5
    pts = torch.cat([p for name, p in sets.items() if name != "vertex y and z"])
    n_rays = pts.shape[0] // N_S
    pts = pts[:n_rays * N_S].contiguous()
    want_off, want_in, want_sd = O.off_in_surface_flags(pts, N_S, fv, 0.05)
    sd = indexed(pts.cuda(), fv.reshape(-1, 9).cuda())
    off = torch.empty(n_rays, dtype=torch.uint8, device="cuda"); inn = torch.empty(n_rays, dtype=torch.uint8, device="cuda")
    hip.lib().mp_mesh_ray_flags(sd, n_rays, N_S, 0.05, off, inn, hip.stream())
    err = (sd.cpu().double() - want_sd.reshape(-1)).abs()
    print(f"[parity] indexed signed distance vs float64: max {err.max().item():.3e} over {pts.shape[0]} points")
    assert err.max() < 1e-5
    m = want_sd.min(1)[0]
    decided = ((m - 0.05).abs() > 1e-5) & (m.abs() > 1e-5)
    assert decided.sum() > 0.5 * n_rays
    assert torch.equal(off.cpu().bool()[decided], want_off[decided]) and torch.equal(inn.cpu().bool()[decided], want_in[decided])


def test_cache_follows_in_place_edits_and_replaced_tensors(sphere3):
    from multiply_amd import hip
    v, f, sets = sphere3
    pts = sets["mix"].cuda().contiguous()
    meshes = [v[f][None].cuda().contiguous()]                    # like model.mesh_face_vertices_list
    cache = hip.MeshIndexCache()
    first = cache.get(0, meshes[0])
    assert bits_equal(first.signed_distance(pts), brute(pts, meshes[0].reshape(-1, 9)))
    assert cache.get(0, meshes[0]) is first                      # unchanged source: the same index
    meshes[0].mul_(1.1)                                          # in place
    second = cache.get(0, meshes[0])
    assert second is not first
    want = brute(pts, meshes[0].reshape(-1, 9))
    assert bits_equal(second.signed_distance(pts), want) and not torch.equal(want, first.signed_distance(pts))
    meshes[0] = (v[f][None] * torch.tensor([0.8, 1.0, 1.2])).cuda().contiguous()      # item replaced
    third = cache.get(0, meshes[0])
    assert third is not second
    assert bits_equal(third.signed_distance(pts), brute(pts, meshes[0].reshape(-1, 9)))
    # hip.mesh_signed_distance with an index = without
    assert bits_equal(hip.mesh_signed_distance(pts, meshes[0][0], index=third), hip.mesh_signed_distance(pts, meshes[0][0]))


def test_auto_builds_an_index_only_for_closed_surfaces_of_enough_faces():
    from multiply_amd import hip
    cache = hip.MeshIndexCache()
    v, f = squashed(4, base=8)                                   # 2 048 faces, closed
    fv, fd = v[f][None].cuda().contiguous(), f.cuda()
    assert isinstance(cache.get(0, fv, fd, "auto"), hip.MeshIndex)
    assert cache.get(0, fv, fd, "brute") is None and isinstance(cache.get(0, fv, None, "index"), hip.MeshIndex)
    assert cache.get(0, fv, None, "auto") is None                # nothing known about the faces
    g = torch.Generator().manual_seed(0)
    soup = torch.randint(0, v.shape[0], (2048, 3), generator=g)  # like the synthetic SMPL tables' face list: no surface
    assert cache.get(1, v[soup][None].cuda().contiguous(), soup.cuda(), "auto") is None
    v3, f3 = squashed(3, base=8)                                 # 512 faces: closed, but too few
    assert cache.get(2, v3[f3][None].cuda().contiguous(), f3.cuda(), "auto") is None


def test_training_forward_flags_are_equal_under_index_and_brute():
    from tests.test_train_step_gpu import _train_setup
    model, oracle, inp, gin, gt, loss_fn, train = _train_setup(epoch=101)
    R = inp["uv"].shape[1]
    v, f = icosphere(3, radius=0.45)
    for p in range(2):
        model.mesh_v_cano_list[p] = v[None].cuda()
        model.mesh_f_cano_list[p] = f.cuda()
        model.mesh_face_vertices_list[p] = v[f][None].cuda()
    hit = [torch.arange(R), torch.arange(R)]
    runs = {}
    for mode in ("index", "brute"):
        model.mesh_index_mode = mode
        torch.manual_seed(11)                                    # the forward draws its sample jitter and eikonal points
        out = model({**gin, "hit_index": hit})
        graph = model._last_train
        runs[mode] = (out["index_off_surface"].clone(), out["index_in_surface"].clone(),
                      [graph.fg[p]["flags"][2].clone() for p in range(2)], [graph.fg[p]["X"].clone() for p in range(2)])
    assert len(model.mesh_index_cache.slots) == 2
    (off_i, in_i, sd_i, x_i), (off_b, in_b, sd_b, x_b) = runs["index"], runs["brute"]
    assert all(torch.equal(a, b) for a, b in zip(x_i, x_b)), "the two forwards did not sample the same points"
    assert off_i.dtype == torch.bool and off_i.shape == (R,)
    assert torch.equal(off_i, off_b) and torch.equal(in_i, in_b)
    assert all(torch.equal(a, b) for a, b in zip(sd_i, sd_b))
    assert off_b.sum() > 0 and in_b.sum() > 0
    with pytest.raises(ValueError):
        model.mesh_index_mode = "bvh"


def test_fit_targets_and_interpenetration_are_equal_under_index_and_brute():
    from multiply_amd import mesh_losses, smpl_init
    v, f = squashed(3)
    cfg = smpl_init.FitConfig()
    gen = torch.Generator(device="cuda").manual_seed(1)
    draws = smpl_init.make_draws(cfg, gen, "cuda")
    dist = {}
    for mode in ("index", "brute"):
        target = smpl_init.MeshTarget(v, f, "cuda", mesh_index_mode=mode)
        assert (target.index is not None) == (mode == "index")
        box = smpl_init.fit_box(cfg, target.verts, "cuda")
        dist[mode] = smpl_init.fit_step_points(target, cfg, box, draws)[3].clone()
    assert torch.equal(dist["index"], dist["brute"]) and (dist["brute"] < 0).any() and (dist["brute"] > 0).any()
    # two overlapping spheres: vertices of each inside the other
    va, vb = v[None].cuda(), (v + torch.tensor([0.25, 0.1, 0.0]))[None].cuda()
    faces = [f[None].cuda(), f[None].cuda()]
    ids = [torch.arange(v.shape[0]), torch.arange(v.shape[0])]
    loss = {mode: mesh_losses.interpenetration_loss([va, vb], faces, draws=ids, mesh_index_mode=mode) for mode in ("index", "brute")}
    assert torch.equal(loss["index"], loss["brute"]) and loss["brute"].item() > 0
