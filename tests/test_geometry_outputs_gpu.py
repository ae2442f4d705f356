"""Volume-rendered depth outputs on the device: mp_composite_geometry through the C ABI, Multiply.render_geometry /
render_views end to end, and the instance masks of mesh_losses.frame_instance_masks(source='volume') against the mesh path.

The reference is tests/geometry_reference.py (float64, sorts the merged list); the bounds are tests/tolerances_geometry.py.
A level crossing is EXACT (same sample: front_person, the -1 pattern, the interpolated depth within its bound) unless the
ray is exempt: the reference's crossing sample is almost empty (fe < 1e-3) or some sample's E + fe lies within 1e-4 of L.
On an exempt ray the device's depth must still lie inside the crossing sample or one of its neighbours in merged order, and at
most 5 % of the rays with a crossing may be exempt."""
import functools

import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import tolerances_geometry as TOL
from tests.util import t32

pytestmark = pytest.mark.gpu

ORDER = ("depth", "depth_person", "depth_level", "front_person", "acc_solo", "depth_solo", "depth_solo_level")
POISON = 777.0
SHAPES = [(70, 3, 98),      # S = 97: one full 64-lane chunk plus a tail of 33
          (5, 1, 65),       # S = 64: exactly one chunk
          (9, 2, 34),       # S = 33, below one chunk
          (13, 8, 130)]     # three chunks at the person limit
MEASURED = {}               # running maxima, printed by every test that measures


def launch(R, inv, z, sdf, beta, level, want=ORDER, guard=0):
    """mp_composite_geometry on numpy inputs -> {name: device buffer with `guard` poisoned rows past n_rays}"""
    from multiply_amd import hip
    L = hip.lib()
    P, NZ = len(inv), z[0].shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [[dev(a) for a in arrs] for arrs in (inv, z, sdf)]
    tabs = [hip.device_ints([t.data_ptr() for t in ts], "cuda") for ts in keep]
    beta_d = torch.tensor([beta], dtype=torch.float32, device="cuda")
    cols = dict(depth=(), depth_person=(P,), depth_level=(), front_person=(), acc_solo=(P,), depth_solo=(P,), depth_solo_level=(P,))
    bufs = {k: torch.full((R + guard,) + cols[k], POISON, dtype=torch.int32 if k == "front_person" else torch.float32,
                          device="cuda") for k in ORDER}
    L.mp_composite_geometry(R, P, NZ, *tabs, beta_d, level, *[bufs[k] if k in want else None for k in ORDER], hip.stream())
    torch.cuda.synchronize()
    return bufs


def _hits(R, P):
    """ray 0 hit by nobody, ray 1 by person 0 alone, the rest by all persons or by a ragged subset"""
    if (R, P) == (70, 3):
        return G.RAGGED_HITS
    return [np.arange(1, R)] + [np.array([r for r in range(2, R) if (r + n) % 5 != 0]) for n in range(1, P)]


@functools.lru_cache(maxsize=None)
def case(shape, beta, level):
    R, P, NZ = shape
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=4, hits=_hits(R, P))
    return inv, z, sdf, G.geometry_reference(R, inv, z, sdf, beta, level)


def _note(name, value):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(value))


def _level_check(tag, got, front, ref_lvl, ref_front, fe_cross, margin, slope, near, near_last):
    """flat arrays over rays (merged) or over (ray, person) pairs (solo) -> (crossings, exempt crossings)"""
    ex = G.exempt(fe_cross, margin)
    cross = ref_lvl >= 0
    n_ex = int((ex & cross).sum())
    for j in np.nonzero(~ex)[0]:
        assert (got[j] == -1) == (not cross[j]), (tag, j, got[j], ref_lvl[j])
        if front is not None:
            assert front[j] == ref_front[j], (tag, j, front[j], ref_front[j])
        if cross[j]:
            err, ceil = abs(float(got[j]) - ref_lvl[j]), TOL.CEIL_LEVEL[0] + TOL.CEIL_LEVEL[1] * slope[j]
            _note("level depth |err|", err)
            _note("level depth |err| / ceiling", err / ceil)
            assert err <= TOL.LEVEL[0] + TOL.LEVEL[1] * slope[j], (tag, j, got[j], ref_lvl[j], err, slope[j])
    for j in np.nonzero(ex)[0]:
        if got[j] == -1:
            assert near_last[j], (tag, j, ref_lvl[j])
        else:
            assert np.isfinite(got[j]) and any(a - 1e-6 <= got[j] <= b + 1e-6 for a, b in near[j]), (tag, j, got[j], near[j])
    return int(cross.sum()), n_ex


def compare(tag, got, ref, inv):
    """every output against the reference under the bounds of tests/tolerances_geometry.py -> (crossings, exempt) merged + solo"""
    g = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in got.items()}
    R, P = ref["depth_person"].shape
    for k in ORDER:
        assert np.isfinite(g[k][:R]).all(), (tag, k)
    hitm = np.stack([np.asarray(iv) >= 0 for iv in inv], 1)
    e_acc = np.abs(g["acc_solo"][:R] - ref["acc_solo"]).max()
    e_dep = max(np.abs(g["depth"][:R] - ref["depth"]).max(), np.abs(g["depth_person"][:R] - ref["depth_person"]).max(),
                np.abs(g["depth_solo"][:R] - ref["depth_solo"]).max())
    _note("opacity |err|", e_acc)
    _note("depth sum |err|", e_dep)
    assert e_acc <= TOL.ACC and e_dep <= TOL.DEPTH, (tag, e_acc, e_dep)
    for k in ("depth_person", "acc_solo", "depth_solo"):
        assert (g[k][:R][~hitm] == 0).all(), (tag, k)
    assert (g["depth_solo_level"][:R][~hitm] == -1).all() and (g["depth"][:R][~hitm.any(1)] == 0).all(), tag
    c1, x1 = _level_check(tag + " merged", g["depth_level"][:R], g["front_person"][:R].astype(np.int64), ref["depth_level"],
                          ref["front_person"], ref["fe_cross"], ref["margin"], ref["slope"], ref["near"], ref["near_last"])
    assert ((g["front_person"][:R] == -1) == (g["depth_level"][:R] == -1)).all(), tag
    assert ((g["front_person"][:R] >= -1) & (g["front_person"][:R] < P)).all(), tag
    flat = lambda a: np.asarray(a).reshape(R * P)
    near_solo = [ref["near_solo"][r][n] for r in range(R) for n in range(P)]
    c2, x2 = _level_check(tag + " solo", flat(g["depth_solo_level"][:R]), None, flat(ref["depth_solo_level"]), None,
                          flat(ref["fe_cross_solo"]), flat(ref["margin_solo"]), flat(ref["slope_solo"]), near_solo,
                          flat(ref["near_last_solo"]))
    return c1, x1, c2, x2


def _report():
    print("[geometry] measured maxima so far:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


# ------------------------------------------------------------------------------------------------ 1. kernel vs reference
@pytest.mark.parametrize("beta,level", [(0.1, 0.5), (0.02, 0.5), (0.001, 0.5), (0.1, 0.9), (0.02, 0.9), (0.001, 0.9)])
def test_kernel_against_the_float64_reference(beta, level):
    tot = np.zeros(4, dtype=np.int64)
    for shape in SHAPES:
        inv, z, sdf, ref = case(shape, beta, level)
        got = launch(shape[0], inv, z, sdf, beta, level)
        cnt = np.array(compare(f"{shape} beta {beta} level {level}", got, ref, inv))
        if shape == SHAPES[0]:
            print(f"[geometry] {shape} beta {beta} level {level}: exempt {cnt[1]} of {cnt[0]} merged, {cnt[3]} of {cnt[2]} solo crossings")
            assert cnt[1] <= 0.05 * cnt[0] and cnt[3] <= 0.05 * cnt[2], cnt
        tot += cnt
    _report()
    assert tot[0] > 0 and tot[2] > 0 and tot[1] <= 0.05 * tot[0] and tot[3] <= 0.05 * tot[2], tot


def test_constructed_rows():
    """ties between identical depth rows, empty rays, a first sample that is already opaque, samples without free energy around
    the crossing"""
    # (a) two persons with identical z rows: every t_end ties, the lower column comes first
    R, P, NZ = 7, 2, 98
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=11)
    z[1] = z[0].copy()
    ref = G.geometry_reference(R, inv, z, sdf, 0.02, 0.5)
    got = launch(R, inv, z, sdf, 0.02, 0.5)
    compare("tied rows", got, ref, inv)
    swapped = G.geometry_reference(R, inv, z, sdf[::-1], 0.02, 0.5)                # what 'higher column first' would give
    d = got["depth_person"].cpu().numpy().astype(np.float64)
    assert np.abs(swapped["depth_person"][:, ::-1] - ref["depth_person"]).max() > 1e-2
    assert np.abs(d - ref["depth_person"]).max() <= TOL.DEPTH

    # (b)-(d) at beta = 0.001, where sdf = +1 has exactly no density and sdf = -1 the full 1 / beta
    R, P, NZ, beta = 7, 2, 34, 0.001
    S = NZ - 1
    inv, z, sdf = G.ragged_case(R, P, NZ, seed=12)
    grid = (1.0 + 0.05 * np.arange(NZ)).astype(np.float32)
    sdf[0][0], sdf[1][0] = 1.0, 1.0                                                # ray 0: empty for both
    sdf[0][1], sdf[1][1] = -1.0, 1.0                                               # ray 1: person 0 opaque in its first sample
    z[0][2], z[1][2] = grid.copy(), grid + 0.02                                    # ray 2: fe == 0 around the crossing
    z[0][2, 11] = z[0][2, 10] + 0.0005                                             #   sample 10: fe = 0.5 < L, then five empty samples
    sdf[0][2], sdf[1][2] = 1.0, 1.0                                                #   of person 0 and person 1's empty ones in between,
    sdf[0][2, 10], sdf[0][2, 16] = -1.0, -1.0                                      #   sample 16 crosses
    z[0][3] = grid.copy()                                                          # ray 3: repeated depths (dt = 0) around the crossing:
    z[0][3, 9:12] = z[0][3, 8]                                                     #   samples 8..10 are empty and tie with sample 7's
    z[0][3, 13] = z[0][3, 12]                                                      #   t_end; sample 11 = [z8, z12] crosses; 12 is empty
    sdf[0][3] = 1.0
    sdf[0][3, 8:13] = -1.0
    sdf[1][3] = 1.0
    ref = G.geometry_reference(R, inv, z, sdf, beta, 0.5)
    got = launch(R, inv, z, sdf, beta, 0.5)
    compare("constructed", got, ref, inv)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert g["depth_level"][0] == -1 and g["front_person"][0] == -1 and g["depth"][0] == 0
    assert (g["acc_solo"][0] == 0).all() and (g["depth_solo"][0] == 0).all() and (g["depth_solo_level"][0] == -1).all()
    assert g["front_person"][1] == 0 and z[0][1, 0] < g["depth_level"][1] < z[0][1, 1]
    assert g["depth_solo_level"][1, 0] == g["depth_level"][1] and g["depth_solo_level"][1, 1] == -1
    assert g["front_person"][2] == 0 and z[0][2, 16] <= g["depth_level"][2] <= z[0][2, 17]
    assert ref["fe_cross"][2] > 1 and ref["fe_cross"][3] > 1 and not G.exempt(ref["fe_cross"], ref["margin"])[:4].any()
    assert g["front_person"][3] == 0 and abs(float(g["depth_level"][3]) - ref["depth_level"][3]) < 1e-4
    _report()


# ------------------------------------------------------------------------------------------------ 2. skipped and untouched memory
def test_null_outputs_are_skipped_and_guard_rows_untouched():
    shape, beta, level = SHAPES[0], 0.02, 0.5
    inv, z, sdf, ref = case(shape, beta, level)
    R = shape[0]
    full = launch(R, inv, z, sdf, beta, level, guard=5)
    again = launch(R, inv, z, sdf, beta, level, guard=5)
    for k in ORDER:
        assert torch.equal(full[k], again[k]), k                                  # bit-identical from run to run
        assert (full[k][R:] == POISON).all(), k                                   # rows past n_rays
        assert not (full[k][:R] == POISON).any(), k
    for want in (("depth_solo_level",), ("depth", "front_person"), ("depth_person", "acc_solo", "depth_solo", "depth_level"), ()):
        part = launch(R, inv, z, sdf, beta, level, want=want, guard=5)
        for k in ORDER:
            if k in want:
                assert torch.equal(part[k], full[k]), (want, k)
            else:
                assert (part[k] == POISON).all(), (want, k)                       # never handed to the kernel: a NULL pointer was
    # fewer rays than the tables hold: only the first n_rays rows are written
    few = launch(R - 3, inv, z, sdf, beta, level, guard=3)
    for k in ORDER:
        assert torch.equal(few[k][:R - 3], full[k][:R - 3]) and (few[k][R - 3:] == POISON).all(), k


# ------------------------------------------------------------------------------------------------ 3. argument checks
def test_argument_errors_make_no_launch():
    inv, z, sdf = G.ragged_case(5, 9, 34, seed=1)
    with pytest.raises(RuntimeError, match="mp_composite_geometry failed with code -1"):
        launch(5, inv, z, sdf, 0.02, 0.5)
    inv, z, sdf = G.ragged_case(5, 2, 34, seed=1)
    for bad in (1.0, 0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="mp_composite_geometry failed with code -3"):
            launch(5, inv, z, sdf, 0.02, bad)
    inv, z, sdf = G.ragged_case(2, 8, 3000, seed=1)                               # 4 waves x 8 persons x 3 x 2999 floats of LDS
    with pytest.raises(RuntimeError, match="mp_composite_geometry failed with code -2"):
        launch(2, inv, z, sdf, 0.02, 0.5)
    out = launch(0, inv[:1], z[:1], sdf[:1], 0.02, 0.5, guard=2)                  # n_rays = 0: status 0, nothing written
    assert all((out[k] == POISON).all() for k in ORDER)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. end to end
GEO_KEYS = ("depth_values", "depth_person_list", "depth_level_values", "front_person", "acc_person_solo_list",
            "depth_person_solo_list", "depth_person_solo_level_list")
BASE_KEYS = ("acc_map", "acc_person_list", "rgb_values", "fg_rgb_values", "normal_values")


def build(P=2, H=20, W=20, seed=0):
    import warnings
    warnings.filterwarnings("ignore")
    from multiply_amd.config import load_config
    from multiply_amd.multiply import Multiply
    from multiply_amd.synthetic import make_scene, make_smpl_tables
    tables = make_smpl_tables(0)
    sc = make_scene(P, seed=seed, H=H, W=W)
    opt = load_config()
    torch.manual_seed(0)
    model = Multiply(opt, sc["smpl_params"][0, :, 76:], smpl_tables=tables).eval()
    sp = t32(sc["smpl_params"])
    inp = dict(uv=t32(sc["uv"]), intrinsics=t32(sc["intrinsics"]), pose=t32(sc["pose"]), smpl_params=sp,
               smpl_pose=sp[:, :, 4:76], smpl_shape=sp[:, :, 76:], smpl_trans=sp[:, :, 1:4], idx=torch.tensor([3]))
    return model, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}


def same_bits(a, b):
    """torch.equal that also holds for the NaN of the ray through the sphere centre (test_render_gpu.report)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _as_launch(out):
    names = dict(zip(ORDER, GEO_KEYS))
    return {k: out[names[k]] for k in ORDER}


def _reference_of_last(model, persons, level):
    per, S = model._last["per"], None
    inv, z, sdf = [], [], []
    for p in persons:
        zz = per[p]["zfinal"].cpu().numpy()
        S = zz.shape[1] - 1
        inv.append(per[p]["inv_index"].cpu().numpy())
        z.append(zz)
        sdf.append(per[p]["sdf"].cpu().numpy().reshape(-1, S)[:zz.shape[0]])
    beta = float(model._beta_value())
    return inv, G.geometry_reference(len(inv[0]), inv, z, sdf, beta, level)


def test_render_geometry_end_to_end():
    model, gin = build(P=2, H=20, W=20)
    R = gin["uv"].shape[1]
    off = model(gin)
    assert set(off) == set(BASE_KEYS)
    off = {k: v.clone() for k, v in off.items()}
    model.render_geometry = True
    on = model(gin)
    torch.cuda.synchronize()
    assert set(on) == set(BASE_KEYS) | set(GEO_KEYS)
    for k in BASE_KEYS:
        assert same_bits(on[k], off[k]), k
    assert on["front_person"].dtype == torch.int32 and on["depth_person_list"].shape == (R, 2) and on["depth_values"].shape == (R,)
    # against the reference on the device's own per-person arrays: hit order, inv_index and the column order
    inv, ref = _reference_of_last(model, [0, 1], 0.5)
    cnt = compare("end to end", _as_launch(on), ref, inv)
    print(f"[geometry] end to end: exempt {cnt[1]} of {cnt[0]} merged, {cnt[3]} of {cnt[2]} solo crossings")
    assert cnt[0] > 20 and cnt[1] <= 0.05 * cnt[0] and cnt[3] <= 0.05 * cnt[2]
    e = (on["acc_person_solo_list"].double().cpu().numpy() >= ref["acc_person"] - 1e-4)
    assert e.all()                                                                  # nobody is more visible behind somebody than alone
    # another level; one person alone has one column
    model.geometry_level = 0.9
    one = model(gin, id=1)
    torch.cuda.synchronize()
    assert one["depth_person_solo_level_list"].shape == (R, 1) and one["acc_person_list"].shape == (R, 1)
    inv1, ref1 = _reference_of_last(model, [1], 0.9)
    compare("person 1 alone, level 0.9", _as_launch(one), ref1, inv1)
    model.geometry_level = 0.5
    # render_views: view n IS person n alone
    views = model.render_views(gin)
    torch.cuda.synchronize()
    assert sorted(views) == [-1, 0, 1] and all(set(v) == set(BASE_KEYS) | set(GEO_KEYS) for v in views.values())
    for k in GEO_KEYS + BASE_KEYS:
        assert same_bits(views[-1][k], on[k]), k
    for n in (0, 1):
        e_acc = float((views[n]["acc_map"] - views[-1]["acc_person_solo_list"][:, n]).abs().max())
        e_dep = float((views[n]["depth_values"] - views[-1]["depth_person_solo_list"][:, n]).abs().max())
        e_lvl = float((views[n]["depth_level_values"] - views[-1]["depth_person_solo_level_list"][:, n]).abs().max())
        print(f"[geometry] view {n} vs the solo columns of view -1: acc {e_acc:.2e}, depth {e_dep:.2e}, level depth {e_lvl:.2e}")
        assert e_acc <= TOL.ACC and e_dep <= TOL.DEPTH
        assert views[n]["depth_person_list"].shape == (R, 1)
    # the flag off gives today's five keys again
    model.render_geometry = False
    assert set(model.render_views(gin)[-1]) == set(BASE_KEYS)
    # a person moved off screen: no ray meets its box (the cull then keeps ray 0 for it, multiply.py:262-263)
    model.render_geometry = True
    far = dict(gin)
    sp = gin["smpl_params"].clone()
    sp[0, 1, 1] += 40.0
    far.update(smpl_params=sp, smpl_trans=sp[:, :, 1:4].contiguous())
    out = model(far)
    torch.cuda.synchronize()
    away = model._last["per"][1]["inv_index"] < 0
    assert int(away.sum()) >= R - 1
    assert (out["depth_person_solo_level_list"][away, 1] == -1).all() and (out["front_person"][away] != 1).all()
    for k in ("acc_person_solo_list", "depth_person_solo_list", "depth_person_list"):
        assert (out[k][away, 1] == 0).all() and torch.isfinite(out[k]).all(), k
    assert bool((out["front_person"] == 0).any())
    _report()


# ------------------------------------------------------------------------------------------------ 5. the consumer
# the share of pixels on which the volume and the mesh path name the same front person, measured on the MI355X
# against the mesh path (9 of 9 and 14 of 14 pixels in two runs: the two bodies of this scene overlap on few pixels at 48 x 48, and
# the fit is not run-to-run identical); the test asserts it minus two percentage points
FRONT_AGREEMENT = 1.0


def fitted_scene(H, W, steps=300):
    """The synthetic two-person scene with its SDF networks fitted to the synthetic body (a short smpl_init fit of person 0,
    shared by both persons like a smpl_init file) and a sharp density, beta = 0.01; the camera matrix and image size the
    mesh path reads.  With the random initialisation the comparison below has no subject: that level set is a sphere of radius
    ~0.6, of which the mesh path rasterises the whole front and the volume renderer only sees what lies within 0.1 of the
    posed body (test_raster_gpu), 14 to 34 lattice cells behind it (measured: medians 33.6 / 14.2 cells, agreement 0.24)."""
    from multiply_amd import smpl_init as S
    from multiply_amd.synthetic import closed_body_mesh
    model, gin = build(P=2, H=H, W=W)
    v, f = closed_body_mesh(model.smpl_server_list[0])
    net = model.foreground_implicit_network_list[0]
    rec = S.fit_implicit_net(net, v, f, cfg=S.FitConfig(n_surface=2048, n_volume=2048, steps=steps))
    model.foreground_implicit_network_list[1].load_state_dict(net.state_dict())
    Kp = gin["intrinsics"][0].double().clone()
    Kp[0, 2] += 0.5; Kp[1, 2] += 0.5                      # the volume renderer shoots rays through integer (x, y)
    gin["P"] = (Kp @ torch.linalg.inv(gin["pose"][0].double()))[None].float()
    gin["img_size"] = (H, W)
    with torch.no_grad():
        model.density.beta.fill_(0.01)
    return model, gin, rec


def test_instance_masks_from_the_volume_against_the_mesh_path():
    """The synthetic two-person scene (networks fitted to the body: fitted_scene) at beta = 0.01, 48 x 48: the unoccluded level
    depths of the volume renderer, converted to z, against the z-buffers of the posed canonical meshes (extraction lattice
    128^3: cell = 1.1 * bounding-box edge / 128)."""
    from multiply_amd import mesh_losses as ML
    H = W = 48
    model, gin, rec = fitted_scene(H, W)
    print(f"[geometry] {rec}")
    m_mesh, d_mesh, k_mesh = ML.frame_instance_masks(model, gin, use_smpl_mesh=False)
    m_vol, d_vol, k_vol = ML.frame_instance_masks(model, gin, use_smpl_mesh=False, source="volume")
    maps, acc = ML.volume_depth_maps(model, gin, level=0.5)
    torch.cuda.synchronize()
    assert m_vol.shape == (2, H, W) and m_vol.dtype == torch.bool and torch.equal(k_mesh, k_vol)
    assert all(torch.equal(a, b) for a, b in zip(maps, d_vol)) and acc.shape == (2, H, W)
    assert not bool((m_vol[0] & m_vol[1]).any()) and bool(m_vol[0].any()) and bool(m_vol[1].any())
    for p in range(2):                                     # a level depth exists exactly where the solo opacity reaches the level
        assert bool(((d_vol[p] >= 0) == (acc[p] >= 0.5 - 1e-4))[(acc[p] - 0.5).abs() > 1e-4].all())
    cells = []
    for p in range(2):
        vc = model.smpl_server_list[p].verts_c[0]
        cells.append(1.1 * float((vc.max(0).values - vc.min(0).values).max()) / 128)
    cell = max(cells)
    # t -> z: the ray's unit direction against the camera axis, over the SMPL scale (get_renderer folds it into the projection)
    cosine = (model._last["dirs"] @ gin["pose"][0, :3, 2]).reshape(H, W) / float(gin["smpl_params"][0, 0, 0])
    zv = [torch.where(d >= 0, d * cosine, d) for d in d_vol]
    med = []
    for p in range(2):
        both = (zv[p] >= 0) & (d_mesh[p] > 0)
        dz = (zv[p] - d_mesh[p]).abs()[both]
        med.append(float(dz.median()) / cells[p])
        print(f"[geometry] person {p}: {int(both.sum())} pixels covered by both (mesh {int((d_mesh[p] > 0).sum())}, volume "
              f"{int((zv[p] >= 0).sum())}), |z volume - z mesh| median {med[-1]:.2f} cells, 90 % {float(dz.quantile(0.9)) / cells[p]:.2f} cells")
        assert int(both.sum()) > 50
    clear = (d_mesh[0] > 0) & (d_mesh[1] > 0) & ((d_mesh[0] - d_mesh[1]).abs() > 4 * cell)
    same = (m_vol[0] == m_mesh[0]) & (m_vol[1] == m_mesh[1])
    share = float(same[clear].float().mean()) if int(clear.sum()) else float("nan")
    print(f"[geometry] front person: volume and mesh path agree on {share:.4f} of the {int(clear.sum())} pixels where the meshes' "
          f"depths differ by more than 4 cells")
    assert max(med) <= 2.0, med
    assert int(clear.sum()) > 0 and FRONT_AGREEMENT is not None and share >= FRONT_AGREEMENT - 0.02, (share, FRONT_AGREEMENT)
