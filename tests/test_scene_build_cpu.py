"""multiply_amd.scene_build on the host: the camera-space -> scene-space transform, the normalisation, the small functions between
detector output and refine_sequence, and the header / binding of the four kernels -- against the float64 restatement
(tests/scene_build_reference.py) and first-principles properties.  Bounds: tests/tolerances_scene_build.py."""
import os
import re

import numpy as np
import pytest

from multiply_amd import scene_build as SB
from tests import scene_build_reference as R
from tests import tolerances_scene_build as TOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mp_raster_mask_batch", "mp_mask_dilate", "mp_mask_stats", "mp_verts_bounds")


def _rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


# ------------------------------------------------------------------------------------------------ transform
def test_rotation_vector_pair_of_the_restatement_round_trips():
    rs = np.random.RandomState(0)
    for r in [rs.normal(size=3), np.array([1e-7, -2e-7, 5e-7]), np.array([0.0, 0.0, 0.0]), (np.pi - 5e-4) * np.array([0.6, 0.0, 0.8])]:
        M = R.rotvec_to_matrix(r)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14
        assert np.abs(R.rotvec_to_matrix(R.matrix_to_rotvec(M)) - M).max() < 1e-14
        assert np.abs(SB.rotvec_to_matrix(r) - M).max() < 1e-14


@pytest.mark.parametrize("case", ["random", "near-zero", "near-pi", "identity-extrinsic"])
def test_transform_keeps_every_vertex_in_place(smpl_tables, case):
    rs = np.random.RandomState({"random": 1, "near-zero": 2, "near-pi": 3, "identity-extrinsic": 4}[case])
    T = R.tables64(smpl_tables)
    pose, betas = R.random_pose(7)
    if case == "near-zero":
        pose[:3] = np.array([3e-7, -5e-7, 6e-7])                      # within 1e-6 of no rotation
    if case == "near-pi":
        pose[:3] = (np.pi - 4e-4) * np.array([0.36, 0.48, 0.8])       # angle within 1e-3 of pi
    trans = rs.normal(0, 1, 3) + [0, 0, 4]
    if case == "identity-extrinsic":
        ext, Rc, tc = None, np.eye(3), np.zeros(3)
    else:
        Rc = _rotation(rs)
        tc = -Rc @ trans + [0.3, -0.2, 4.0]                            # the body stays about 4 m in front of the camera
        ext = np.concatenate([Rc, tc[:, None]], 1)
    T_hip = R.t_hip(T, betas)
    pose2, trans2 = SB.to_scene_space(pose[None], trans[None], T_hip[None], ext)
    assert np.array_equal(pose2[0, 3:], pose[3:])
    v, v2 = R.body(T, trans, pose, betas), R.body(T, trans2[0], pose2[0], betas)
    err = np.abs(v2 @ R.RT.T - (v @ Rc.T + tc)).max()
    # against the restatement's own transform
    pr, tr = R.to_scene_space(pose, trans, T_hip, Rc, tc)
    dr = np.abs(R.rotvec_to_matrix(pr[:3]) - R.rotvec_to_matrix(pose2[0, :3])).max()
    print(f"transform {case}: max |Rt v' - (Rc v + tc)| {err:.3e} m, root rotation against the restatement {dr:.3e}, trans {np.abs(tr - trans2[0]).max():.3e}")
    assert err <= TOL.BODY_EPS_METRES and dr <= TOL.HOST_METRES and np.abs(tr - trans2[0]).max() <= TOL.HOST_METRES
    # cam_f on v' + shift_f against K (Rc v + tc), in pixels
    K = np.array([[1400.0, 0, 960.0], [0, 1410.0, 540.0], [0, 0, 1]])
    for s in (1, 2):
        shift = SB.shifts_from_bounds(np.concatenate([v2.min(0), v2.max(0)])[None])
        cam = SB.frame_cameras(SB.intrinsics4(K, s), shift)[0]
        x = (np.concatenate([v2 + shift[0], np.ones((v2.shape[0], 1))], 1)) @ cam.T
        c = v @ Rc.T + tc
        assert c[:, 2].min() >= 2.5
        want = np.stack([K[0, 0] / s * c[:, 0] / c[:, 2] + K[0, 2] / s, K[1, 1] / s * c[:, 1] / c[:, 2] + K[1, 2] / s], 1)
        px = np.abs(x[:, :2] / x[:, 2:3] - want).max()
        print(f"  scale_factor {s}: reprojection {px:.3e} px")
        assert px <= TOL.BODY_EPS_PIXELS


def test_to_scene_space_broadcasts_over_frames_and_persons(smpl_tables):
    rs = np.random.RandomState(5)
    pose, trans, th = rs.normal(0, 0.5, (3, 2, 72)), rs.normal(0, 1, (3, 2, 3)), rs.normal(0, 0.2, (2, 3))
    ext = np.concatenate([_rotation(rs), rs.normal(size=(3, 1))], 1)
    p2, t2 = SB.to_scene_space(pose, trans, th[None], ext)
    for f in range(3):
        for p in range(2):
            pr, tr = R.to_scene_space(pose[f, p], trans[f, p], th[p], ext[:, :3], ext[:, 3])
            assert np.abs(R.rotvec_to_matrix(pr[:3]) - R.rotvec_to_matrix(p2[f, p, :3])).max() <= TOL.HOST_METRES
            assert np.abs(tr - t2[f, p]).max() <= TOL.HOST_METRES


# ------------------------------------------------------------------------------------------------ normalisation
def _hand_set():
    """two persons, three frames: the extremes of every frame's vertices by hand"""
    lo = np.array([[-1.0, -2.0, 3.0], [-0.5, -1.0, 2.0], [0.0, -3.0, 1.0]])
    hi = np.array([[3.0, 0.0, 5.0], [1.5, 1.0, 6.0], [2.0, 1.0, 2.0]])
    return np.concatenate([lo, hi], 1)


def test_shift_per_frame_and_first_frame():
    b = _hand_set()
    per = SB.shifts_from_bounds(b, "per_frame")
    assert np.array_equal(per, np.array([[-1.0, 1.0, -4.0], [-0.5, 0.0, -4.0], [-1.0, 1.0, -1.5]]))
    first = SB.shifts_from_bounds(b, "first_frame")
    assert np.array_equal(first, np.tile([[-1.0, 1.0, -4.0]], (3, 1)))
    with pytest.raises(ValueError, match="normalize"):
        SB.shifts_from_bounds(b, "hi4d")


@pytest.mark.parametrize("branch", ["camera-farther", "bodies-farther"])
@pytest.mark.parametrize("s", [1, 2])
def test_normalize_cameras_by_hand(branch, s):
    from multiply_amd.datasets import load_K_Rt_from_P
    K = np.array([[1400.0, 0, 960.0], [0, 1410.0, 540.0], [0, 0, 1]])
    shift = SB.shifts_from_bounds(_hand_set())
    cams = SB.frame_cameras(SB.intrinsics4(K, s), shift)
    far = np.linalg.norm(shift, axis=1).max()                      # |(-1, 1, -4)| = sqrt(18)
    assert far == np.sqrt(18.0)
    sphere = 1.25 if branch == "camera-farther" else 7.5
    out, r = SB.normalize_cameras(cams, sphere)
    want_r = 1.1 * (far if branch == "camera-farther" else sphere)
    assert abs(r - want_r) <= 1e-12 * want_r
    assert sorted(out) == sorted(["scale_mat_%d" % i for i in range(3)] + ["world_mat_%d" % i for i in range(3)])
    K4 = SB.intrinsics4(K, s)
    for f in range(3):
        sm, wm = out["scale_mat_%d" % f], out["world_mat_%d" % f]
        assert sm.dtype == np.float32 and np.array_equal(sm, np.diag([r / 3, r / 3, r / 3, 1]).astype(np.float32))
        assert np.array_equal(wm, cams[f]) and wm.dtype == np.float64
        # E_f = [Rt | -Rt shift_f]: the camera sits at shift_f
        assert np.abs(np.linalg.inv(K4) @ wm - np.block([[R.RT, (-R.RT @ shift[f])[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])).max() < 1e-12
        intr, pose = load_K_Rt_from_P((wm @ sm)[:3, :4])
        assert np.abs(intr - K4).max() <= TOL.HOST_PIXELS
        assert np.abs(pose[:3, 3] - shift[f] / float(sm[0, 0])).max() <= 4 * np.spacing(np.float32(4.0))      # pose is float32
        assert np.abs(pose[:3, :3] - R.RT.T).max() <= 1e-6
        Kr, cr = R.camera_centre_and_K(wm[:3])
        assert np.abs(Kr - K4[:3, :3]).max() <= TOL.HOST_PIXELS and np.abs(cr - shift[f]).max() <= TOL.HOST_METRES
        assert np.linalg.norm(pose[:3, 3]) <= 3.0 / 1.1 * (1 + 1e-6)


# ------------------------------------------------------------------------------------------------ estimate_translation
@pytest.mark.parametrize("N", [1, 7])
def test_estimate_translation_recovers_exact_projections(N):
    rs = np.random.RandomState(N)
    K = np.array([[1400.0, 0, 960.0], [0, 1380.0, 540.0], [0, 0, 1]])
    X = rs.normal(0, 0.4, (N, 24, 3))
    t = rs.normal(0, 0.5, (N, 3)) + [0, 0, 4.0]
    c = X + t[:, None]
    uv = np.stack([K[0, 0] * c[..., 0] / c[..., 2] + K[0, 2], K[1, 1] * c[..., 1] / c[..., 2] + K[1, 2]], -1)
    got = SB.estimate_translation(X, uv, K)
    assert got.shape == (N, 3) and got.dtype == np.float64
    err = np.abs(got - t).max()
    print(f"estimate_translation N = {N}: max |t - truth| {err:.3e} m")
    assert err <= TOL.HOST_METRES
    # zero-weight joints are ignored: corrupt them and the answer must not move
    w = np.ones((N, 24))
    w[:, ::3] = 0
    base = SB.estimate_translation(X, uv, K, w)
    bad = uv.copy()
    bad[:, ::3] += rs.normal(0, 300, bad[:, ::3].shape)
    Xb = X.copy()
    Xb[:, ::3] += 5.0
    assert np.array_equal(SB.estimate_translation(Xb, bad, K, w), base)
    assert np.abs(base - t).max() <= TOL.HOST_METRES
    assert np.abs(SB.estimate_translation(X, bad, K) - t).max() > 1e-2        # and they do matter when weighted
    with pytest.raises(ValueError):
        SB.estimate_translation(X, uv[:, :5], K)


# ------------------------------------------------------------------------------------------------ interpolate_missing
def _trajectory(F=12):
    rs = np.random.RandomState(3)
    from scipy.spatial.transform import Rotation
    t = np.arange(F, dtype=np.float64)
    pose = np.empty((F, 72))
    for j in range(24):
        r0, rate = Rotation.from_rotvec(rs.normal(0, 0.5, 3)), rs.normal(0, 0.05, 3)          # a constant-rate rotation
        pose[:, 3 * j:3 * j + 3] = (Rotation.from_rotvec(t[:, None] * rate[None]) * r0).as_rotvec()
    c = rs.normal(0, 1, (4, 3)) * np.array([1.0, 0.1, 0.01, 0.001])[:, None]                  # a cubic translation
    trans = c[0] + t[:, None] * c[1] + t[:, None] ** 2 * c[2] + t[:, None] ** 3 * c[3]
    return pose, trans


def _rot_err(a, b):
    return max(np.abs(R.rotvec_to_matrix(x) - R.rotvec_to_matrix(y)).max() for x, y in zip(a.reshape(-1, 3), b.reshape(-1, 3)))


@pytest.mark.parametrize("ids", [(4,), (3, 4, 8), (0,), (11,), (0, 5, 11), (5, 5)], ids=str)
def test_interpolate_missing_recovers_a_smooth_trajectory(ids):
    pose, trans = _trajectory()
    broken_p, broken_t = pose.copy(), trans.copy()
    broken_p[list(ids)] = 9.0
    broken_t[list(ids)] = -7.0
    keep_p, keep_t = broken_p.copy(), broken_t.copy()
    got_p, got_t = SB.interpolate_missing(broken_p, broken_t, ids)
    assert np.array_equal(broken_p, keep_p) and np.array_equal(broken_t, keep_t)             # the inputs are not written
    rest = np.setdiff1d(np.arange(12), ids)
    assert np.array_equal(got_p[rest], pose[rest]) and np.array_equal(got_t[rest], trans[rest])      # bit-unchanged
    ref_p, ref_t = R.interpolate(broken_p, broken_t, np.array(ids))
    sel = sorted(set(ids))
    e_p, e_t = _rot_err(got_p[sel], pose[sel]), np.abs(got_t[sel] - trans[sel]).max()
    r_p, r_t = _rot_err(ref_p[sel], pose[sel]), np.abs(ref_t[sel] - trans[sel]).max()
    print(f"interpolate {ids}: rotation error {e_p:.3e} (the restatement's {r_p:.3e}), translation {e_t:.3e} ({r_t:.3e})")
    # the bound is what the same scipy splines reach in the restatement, plus float64 rounding of values of order 1 - 10
    assert e_p <= r_p + TOL.HOST_METRES and e_t <= r_t + TOL.HOST_METRES
    assert _rot_err(got_p[sel], ref_p[sel]) <= TOL.HOST_METRES
    inside = [i for i in sel if 0 < i < 11]
    if inside:          # inside the available range a cubic translation is reproduced by the (not-a-knot) cubic spline
        assert np.abs(got_t[inside] - trans[inside]).max() <= TOL.HOST_METRES * 10


def test_interpolate_missing_with_no_ids_and_bad_ids():
    pose, trans = _trajectory()
    p, t = SB.interpolate_missing(pose, trans, [])
    assert np.array_equal(p, pose) and np.array_equal(t, trans) and p is not pose
    with pytest.raises(ValueError):
        SB.interpolate_missing(pose, trans, [12])
    with pytest.raises(ValueError):
        SB.interpolate_missing(pose, trans, range(11))


# ------------------------------------------------------------------------------------------------ match_detections
def _detections(rs, centres, spread=15.0, K=25):
    """one detection per centre: keypoints around it whose confidence-weighted mean IS the centre"""
    out = []
    for c in centres:
        kp = np.concatenate([rs.normal(0, spread, (K, 2)), rs.uniform(0.2, 1.0, (K, 1))], 1)
        kp[:, :2] += c - (kp[:, :2] * kp[:, 2:]).sum(0) / kp[:, 2].sum()
        out.append(kp)
    return np.stack(out)


def test_match_detections():
    rs = np.random.RandomState(9)
    cen = np.array([[[100.0, 200.0], [400.0, 220.0], [700.0, 180.0]], [[120.0, 210.0], [390.0, 230.0], [690.0, 170.0]]])
    det0 = _detections(rs, cen[0] + rs.normal(0, 5, (3, 2)))
    perm = [2, 0, 1]
    # frame 0: permuted; frame 1: more detections than persons (a far one extra)
    det1 = _detections(rs, np.concatenate([cen[1] + rs.normal(0, 5, (3, 2)), [[1500.0, 900.0]]]))
    got = SB.match_detections([det0[perm], det1[[3, 1, 0, 2]]], cen)
    assert got.shape == (2, 3, 25, 3) and got.dtype == np.float32
    assert np.array_equal(got[0], det0.astype(np.float32)) and np.array_equal(got[1], det1[:3].astype(np.float32))
    # fewer detections than persons: the unmatched person has a zero row
    got = SB.match_detections([det0[[2, 0]], det1[:0]], cen)
    assert np.array_equal(got[0, 0], det0[0].astype(np.float32)) and np.array_equal(got[0, 2], det0[2].astype(np.float32))
    assert not got[0, 1].any() and not got[1].any()
    # a detection beyond max_cost is dropped, exactly at max_cost too (the test is <)
    far = _detections(rs, cen[0] + np.array([[0.0, 0.0], [0.0, 250.0], [0.0, 0.0]]))
    got = SB.match_detections([far, det1[:3]], cen)
    assert got[0, 0].any() and got[0, 2].any() and not got[0, 1].any()
    assert SB.match_detections([far, det1[:3]], cen, max_cost=400.0)[0, 1].any()
    # an all-zero-confidence detection: no NaN, never matched
    dead = det0.copy()
    dead[1, :, 2] = 0
    got = SB.match_detections([dead, det1[:3]], cen)
    assert np.isfinite(got).all() and not got[0, 1].any() and np.array_equal(got[0, 0], det0[0].astype(np.float32))
    with pytest.raises(ValueError):
        SB.match_detections([det0], cen)


# ------------------------------------------------------------------------------------------------ gate_second_set
@pytest.mark.parametrize("d_right", [29.0, 30.0, 31.0])
@pytest.mark.parametrize("d_left", [12.0, 30.0, 45.0])
def test_gate_second_set(d_left, d_right):
    rs = np.random.RandomState(2)
    first = np.concatenate([rs.uniform(100, 900, (1, 2, 17, 2)), rs.uniform(0.3, 1, (1, 2, 17, 1))], -1)
    second = np.concatenate([rs.uniform(100, 900, (1, 2, 25, 2)), rs.uniform(0.3, 1, (1, 2, 25, 1))], -1).astype(np.float32)
    # person 0 carries the two distances under test (3-4-5 triangles: exact in float), person 1 agrees everywhere
    for p, (dl, dr) in enumerate([(d_left, d_right), (0.0, 0.0)]):
        second[0, p, 14, :2] = first[0, p, 15, :2] = [500.0, 300.0]
        second[0, p, 11, :2] = first[0, p, 16, :2] = [300.0, 500.0]
        first[0, p, 15, :2] += [0.6 * dl, 0.8 * dl]
        first[0, p, 16, :2] -= [0.8 * dr, 0.6 * dr]
    keep = second.copy()
    out = SB.gate_second_set(first, second)
    assert np.array_equal(second, keep) and out.dtype == second.dtype and out.shape == second.shape
    assert np.array_equal(out[..., :2], second[..., :2]) and not out[..., :19, 2].any()
    assert np.array_equal(out[0, 1, 19:, 2], second[0, 1, 19:, 2])
    for foot, d in (((19, 20, 21), d_left), ((22, 23, 24), d_right)):
        want = np.zeros(3) if d > 30.0 else second[0, 0, list(foot), 2]           # exactly 30 px keeps them: the test is >
        assert np.array_equal(out[0, 0, list(foot), 2], want), (foot, d)


# ------------------------------------------------------------------------------------------------ header, binding, docs
def test_header_binding_and_docs():
    from multiply_amd import hip
    protos = hip.header_prototypes()
    hdr = open(hip.HEADER_PATH).read()
    src = open(os.path.join(REPO, "multiply_amd", "csrc", "raster.hip")).read() + open(os.path.join(REPO, "multiply_amd", "csrc", "scene.hip")).read()
    for name in ENTRY_POINTS:
        assert name in protos and name not in hip.VALUE_RETURNING, name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert protos[name][0] is hip.C.c_int and protos[name][1][-1] is hip.DevPtr          # a status; the stream comes last
        assert re.search(r"%s\([^;]*void\* stream\);" % name, hdr), name
    assert [len(protos[n][1]) for n in ENTRY_POINTS] == [12, 10, 6, 6]
    assert protos["mp_verts_bounds"][1][:5] == [hip.DevPtr, hip.C.c_int, hip.C.c_int, hip.DevPtr, hip.DevPtr]
    block = hdr[hdr.index("mp_raster_mask_batch :"):hdr.index("int mp_raster_mask_batch(")]
    for words in ("Status -1 without a launch", "Status -2 without a launch", "N == 0 returns 0", "F == 0 returns 0", "MP_DILATE_MAX_K"):
        assert words in block, words
    assert "#define MP_DILATE_MAX_K 64" in hdr
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "scene_build" in open(os.path.join(REPO, doc)).read(), doc


def test_raster_cases_cover_the_image_partly(smpl_tables):
    """the poses of the device test were chosen so that equality with the z-buffer is not the equality of empty masks: every
    non-degenerate body covers 5 % .. 95 % of the smaller image under the CPU rasteriser, the one behind the camera nothing"""
    from oracle import raster_oracle as RO
    verts, faces = R.raster_bodies(smpl_tables)
    H, W, f = R.RASTER_SIZES[0]
    for i in range(verts.shape[0]):
        z, _, _ = RO.rasterize(verts[i].astype(np.float64), faces, np.eye(3), np.zeros(3), f, f, W / 2, H / 2, H, W, z_clip=SB.Z_CLIP)
        cov = float((z >= 0).mean())
        print(f"body {i} at {R.RASTER_TRANS[i]}: covers {cov:.3f}")
        assert (cov == 0.0) if R.RASTER_TRANS[i][2] < 0 else (0.05 <= cov <= 0.95), i
    uv = verts[1][:, 0] / verts[1][:, 2] * f + W / 2
    assert 0.25 < float((uv >= W).mean()) < 0.75                     # half outside
