"""Pose metrics without a device: the float64 restatement (tests/pose_metrics_reference.py) on analytic anchors, the host-side
pieces of multiply_amd/pose_metrics.py, its argument checks (which must raise before the device is touched) and the command-line
tool's argument handling."""
import os
import re

import numpy as np
import pytest
import torch

from multiply_amd import hip, pose_metrics as PM
from tests import pose_metrics_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def cloud(n=40, seed=0):
    return np.random.RandomState(seed).normal(0, 1, (n, 3)) * np.array([1.0, 0.7, 0.4])


# ------------------------------------------------------------------------------------------------ the restatement's anchors
def test_pure_translation():
    x = cloud()
    t = np.array([0.3, -0.2, 0.6])
    plain, aligned, pa, flag = R.item_errors(x + t, x, (x + t)[0], x[0])
    assert abs(plain - np.linalg.norm(t)) <= 1e-15 and aligned <= 1e-15 and pa <= 1e-14 and flag == 0


def test_known_similarity_is_undone_by_procrustes():
    x = cloud()
    extent = np.abs(x).max()
    p = 1.3 * x @ rotation([1, 2, -1], 0.8).T + np.array([0.5, 0.1, -0.3])
    plain, aligned, pa, _ = R.item_errors(p, x, p[0], x[0])
    assert pa <= 1e-12 * extent and aligned > 0.1 and plain > 0.1
    s, Rm, t = R.umeyama(p, x)
    assert abs(s - 1 / 1.3) <= 1e-13 and abs(np.linalg.det(Rm) - 1) <= 1e-13


def horn(p, x):
    """the best PROPER rotation by Horn's quaternion form (an eigenvector, no SVD and no D), then Umeyama's scale and translation"""
    pc, xc = p - p.mean(0), x - x.mean(0)
    S = pc.T @ xc
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, v = np.linalg.eigh(N)
    q0, q1, q2, q3 = v[:, -1]
    Rm = np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                   [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                   [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])
    s = (xc * (pc @ Rm.T)).sum() / (pc * pc).sum()
    return np.linalg.norm(s * pc @ Rm.T - xc, axis=1).mean()


def test_mirrored_cloud_is_not_aligned():
    x = cloud()
    p = x * np.array([-1.0, 1.0, 1.0])
    pa = R.item_errors(p, x)[2]
    assert pa > 0.1                                                       # strictly positive, far from rounding
    assert abs(pa - horn(p, x)) <= 1e-12                                  # the value under det R = +1, by a route without D
    assert R.item_errors(p, x, constrained=False)[2] <= 1e-12            # an orthogonal fit (a reflection) would give 0
    s, Rm, _ = R.umeyama(p, x)
    assert abs(np.linalg.det(Rm) - 1) <= 1e-13


def test_coplanar_cloud_under_a_rigid_motion():
    x = cloud()
    x[:, 2] = 0.0
    p = x @ rotation([0.3, -1, 0.5], 1.1).T + np.array([0.2, 0.4, -0.1])
    _, _, pa, flag = R.item_errors(x, p)
    assert pa <= 1e-12 and flag == 0
    assert R.item_errors(p, x)[2] <= 1e-12


def test_left_out_items():
    x = cloud(8)
    bad = x.copy()
    bad[3, 1] = np.nan
    assert R.item_errors(bad, x)[3] == 1 and np.isnan(R.item_errors(bad, x)[:3]).all()
    one = np.repeat(x[:1], 8, 0)
    plain, _, pa, flag = R.item_errors(one, x)
    assert flag == 2 and np.isnan(pa) and plain > 0


def two_triangles():
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    verts = np.stack([tri, tri + np.array([0, 0, 1.0])])[None]            # (1, 2, 3, 3): person 1 = person 0 one unit up
    faces = np.array([[0, 1, 2]])
    c = dict(frame=np.array([0, 0, 0]), person_a=np.array([0, 0, 1]), vertex=np.array([0, 1, 2]), person_b=np.array([1, 1, 0]),
             face=np.array([0, 0, 0]), bary=np.array([[1.0, 0, 0], [1 / 3, 1 / 3, 1 / 3], [0, 0.5, 0.5]]))
    # vertex 0 against its own copy: 1; vertex 1 = (1,0,0) against the centroid (1/3,1/3,1): sqrt(4/9 + 1/9 + 1);
    # person 1's vertex 2 = (0,1,1) against the midpoint (1/2,1/2,0) of person 0's edge: sqrt(1/4 + 1/4 + 1)
    return verts, faces, c, np.array([1.0, np.sqrt(14 / 9), np.sqrt(1.5)])


def test_contact_distance_on_two_triangles():
    verts, faces, c, want = two_triangles()
    mean, per, cnt = R.contact_distance(verts, faces, c)
    assert abs(mean - want.mean()) <= 1e-15 and abs(per[0] - want.mean()) <= 1e-15 and cnt.tolist() == [3]
    two = np.concatenate([verts, verts])                                  # a second frame without a correspondence
    mean, per, cnt = R.contact_distance(two, faces, c)
    assert np.isnan(per[1]) and cnt.tolist() == [3, 0] and abs(mean - want.mean()) <= 1e-15


# depths of three persons in two frames, threshold 0.15: pairs (0,1), (0,2), (1,2)
Z_GT = np.array([[1.0, 1.1, 2.0], [3.0, 2.0, 2.5]])
Z_PRED = np.array([[1.0, 1.3, 1.9], [2.0, 2.1, 2.6]])
REL_GT = [[0, -1, -1], [1, 1, -1]]             # frame 0: |1 - 1.1| < 0.15 -> 0
REL_PRED = [[-1, -1, -1], [0, -1, -1]]         # frame 1: |2 - 2.1| < 0.15 -> 0
PCDR = 3 / 6                                   # equal: frame 0 pairs (0,2), (1,2); frame 1 pair (1,2)


def test_pcdr_table():
    assert R.relations(Z_GT, 0.15)[0].tolist() == REL_GT and R.relations(Z_PRED, 0.15)[0].tolist() == REL_PRED
    share, per, n = R.pcdr(Z_PRED, Z_GT, 0.15)
    assert share == PCDR and per.tolist() == [2 / 3, 1 / 3] and n == 6
    assert R.relations(100 * Z_GT, 15.0)[0].tolist() == REL_GT and R.relations(Z_GT, 15.0, unit_scale=100.0)[0].tolist() == REL_GT
    share, per, n = R.pcdr(Z_PRED[:, :1], Z_GT[:, :1], 0.15)
    assert np.isnan(share) and n == 0 and np.isnan(per).all()
    view = np.array([[1.0, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0.5]])      # camera z = 0.5 - world y
    pos = np.zeros((2, 3, 3))
    pos[..., 1] = 0.5 - Z_GT
    assert np.allclose(R.depths(pos, view), Z_GT, atol=1e-15) and np.allclose(R.depths(pos, np.stack([view, view])), Z_GT, atol=1e-15)


# ------------------------------------------------------------------------------------------------ the module's host-side pieces
def test_depth_relations_on_the_table():
    for z, want in ((Z_GT, REL_GT), (Z_PRED, REL_PRED)):
        rel, ok = PM.depth_relations(torch.from_numpy(z).float(), 0.15)
        assert rel.tolist() == want and bool(ok.all())
    rel, ok = PM.depth_relations(torch.tensor([[1.0, float("nan")]]), 0.15)
    assert not bool(ok.any())
    assert PM.depth_relations(torch.zeros(2, 1), 0.15)[0].shape == (2, 0)


def test_closest_barycentrics_in_every_region():
    """interior, the three edges and the three vertices, against the float64 reference of the closest-face tests"""
    from tests import mesh_metrics_reference as MR
    rng = np.random.RandomState(1)
    tri = rng.normal(0, 1, (700, 3, 3))
    tri[:100, 2] = tri[:100, 0] + 1e-4 * rng.normal(0, 1, (100, 3))                     # slivers
    w = rng.dirichlet([1, 1, 1], 700)
    p = (w[:, :, None] * tri).sum(1) + rng.normal(0, 0.3, (700, 3)) * rng.choice([0.01, 1.0, 3.0], (700, 1))
    b = PM.closest_barycentrics(torch.from_numpy(p), torch.from_numpy(tri)).numpy()
    d2, q = MR.closest_points_paired(p, tri)
    got = (b[:, :, None] * tri).sum(1)
    assert np.linalg.norm(got - q, axis=1).max() <= 1e-12 and (b >= 0).all() and np.abs(b.sum(1) - 1).max() <= 1e-15
    zeros = (b == 0).sum(1)
    assert (zeros == 0).sum() > 20 and (zeros == 1).sum() > 20 and (zeros == 2).sum() > 20   # every kind of region was met
    on = PM.closest_barycentrics(torch.from_numpy((w[:, :, None] * tri).sum(1)[100:]), torch.from_numpy(tri[100:])).numpy()
    assert np.abs(on - w[100:]).max() <= 1e-9                                            # a point on the face gets its own coordinates


def test_params_from_body_models():
    from multiply_amd.body_model_params import BodyModelParams
    rng = np.random.RandomState(0)
    models, want = [], np.zeros((5, 2, 86), np.float32)
    for p in range(2):
        bm = BodyModelParams(5)
        data = {k: rng.normal(0, 1, (1 if k == "betas" else 5, d)).astype(np.float32) for k, d in bm.params_dim.items()}
        for k, v in data.items():
            bm.init_parameters(k, torch.from_numpy(v.copy()), requires_grad=True)
        models.append(bm)
        want[:, p, 0], want[:, p, 1:4], want[:, p, 4:7] = 1.1, data["transl"], data["global_orient"]
        want[:, p, 7:76], want[:, p, 76:] = data["body_pose"], data["betas"]
    got = PM.params_from_body_models(models, scale=1.1)
    assert got.shape == (5, 2, 86) and not got.requires_grad and np.array_equal(got.numpy(), want)


def test_constants_equal_the_header():
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    rows, work = (int(re.search(r"#define %s (\d+)" % k, hdr).group(1)) for k in ("MP_SMPL_BATCH_ROWS", "MP_SMPL_BATCH_ROW_WORK"))
    assert (rows, work) == (hip.SMPL_BATCH_ROWS, hip.SMPL_BATCH_ROW_WORK)
    protos = hip.header_prototypes()
    assert len(protos["mp_smpl_pose_batch"][1]) == 14 and len(protos["mp_pose_errors"][1]) == 8 and len(protos["mp_contact_distance"][1]) == 13
    assert not {"mp_smpl_pose_batch", "mp_pose_errors", "mp_contact_distance"} & set(hip.VALUE_RETURNING)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture
def no_device(monkeypatch):
    def touched():
        raise AssertionError("the device was touched before the arguments were checked")
    monkeypatch.setattr(hip, "require_device", touched)
    monkeypatch.setattr(hip, "lib", touched)


def _bodies(F=2, P=2, J=24, V=30, dtype=np.float32):
    rng = np.random.RandomState(0)
    return {"joints": rng.normal(0, 1, (F, P, J, 3)).astype(dtype), "verts": rng.normal(0, 1, (F, P, V, 3)).astype(dtype)}


def _contacts(**over):
    c = dict(frame=np.array([0, 1]), person_a=np.array([0, 1]), vertex=np.array([3, 4]), person_b=np.array([1, 0]),
             face=np.array([0, 1]), bary=np.array([[1.0, 0, 0], [0.2, 0.3, 0.5]]))
    c.update(over)
    return c


FACES = np.array([[0, 1, 2], [3, 4, 5]])


@pytest.mark.parametrize("kwargs, exc, match", [
    (dict(pred=np.zeros((2, 2, 85), np.float32)), ValueError, r"pred: expected parameters \(F, P, 86\)"),
    (dict(pred=np.zeros((2, 2, 86), np.float32)), ValueError, "servers"),
    (dict(pred=np.zeros((2, 2, 86), np.float32), servers=[object()]), ValueError, r"servers: expected one per person \(2\)"),
    (dict(pred=_bodies(dtype=np.float64)), TypeError, r"pred\['joints'\]: expected float32"),
    (dict(gt={"verts": np.zeros((2, 2, 30), np.float32)}), ValueError, r"gt\['verts'\]: expected \(F, P, n, 3\)"),
    (dict(gt={}), ValueError, "gt: a dict needs"),
    (dict(gt=_bodies(F=3)), ValueError, r"pred has \(F, P\)"),
    (dict(gt=_bodies(V=31)), ValueError, "number of vertices"),
    (dict(gt={"joints": _bodies(J=17)["joints"]}), ValueError, "number of joints"),
    (dict(pred={"joints": _bodies()["joints"]}, gt={"verts": _bodies()["verts"]}), ValueError, "neither joints nor vertices"),
    (dict(root=24), ValueError, "root"),
    (dict(unit_scale=0.0), ValueError, "unit_scale"),
    (dict(depth_threshold=-1.0), ValueError, "depth_threshold"),
    (dict(view=np.zeros((3, 3))), ValueError, "view"),
    (dict(joint_regressor=np.zeros((14, 31), np.float32)), ValueError, "joint_regressor"),
    (dict(joint_regressor=np.zeros((14, 30), np.float64)), TypeError, "joint_regressor"),
    (dict(contacts=_contacts()), ValueError, "faces"),
    (dict(contacts=_contacts(), faces=np.array([[0, 1, 30]])), ValueError, "faces: vertex ids"),
    (dict(contacts=_contacts(), faces=FACES.astype(np.float32)), TypeError, "faces"),
    (dict(contacts=_contacts(face=np.array([0, 2])), faces=FACES), ValueError, r"contacts\['face'\]"),
    (dict(contacts=_contacts(person_a=np.array([0, 2])), faces=FACES), ValueError, r"contacts\['person_a'\]"),
    (dict(contacts=_contacts(person_b=np.array([-1, 0])), faces=FACES), ValueError, r"contacts\['person_b'\]"),
    (dict(contacts=_contacts(frame=np.array([0, 2])), faces=FACES), ValueError, r"contacts\['frame'\]"),
    (dict(contacts=_contacts(vertex=np.array([3, 30])), faces=FACES), ValueError, r"contacts\['vertex'\]"),
    (dict(contacts=_contacts(vertex=np.array([3.0, 4.0])), faces=FACES), TypeError, r"contacts\['vertex'\]"),
    (dict(contacts=_contacts(bary=np.zeros((2, 2))), faces=FACES), ValueError, r"contacts\['bary'\]"),
    (dict(contacts={"frame": np.array([0])}, faces=FACES), ValueError, "contacts: expected a dict"),
])
def test_arguments_are_checked_before_the_device_is_touched(no_device, kwargs, exc, match):
    args = dict(pred=_bodies(), gt=_bodies())
    args.update(kwargs)
    with pytest.raises(exc, match=match):
        PM.pose_metrics(**args)


def test_valid_arguments_reach_the_device(no_device):
    with pytest.raises(AssertionError, match="the device was touched"):
        PM.pose_metrics(_bodies(), _bodies(), contacts=_contacts(), faces=FACES, view=np.zeros((2, 3, 4), np.float32))


def test_pose_sequence_and_contacts_check_their_arguments(no_device):
    with pytest.raises(ValueError, match="params"):
        PM.pose_sequence([object()], np.zeros((2, 1, 72), np.float32))
    with pytest.raises(ValueError, match="servers"):
        PM.pose_sequence([object()], np.zeros((2, 2, 86), np.float32))
    with pytest.raises(ValueError, match="faces"):
        PM.contacts_from_bodies(_bodies()["verts"], np.array([[0, 1, 99]]), 0.01)
    with pytest.raises(ValueError, match="threshold"):
        PM.contacts_from_bodies(_bodies()["verts"], FACES, float("nan"))


# ------------------------------------------------------------------------------------------------ the tool
def test_eval_tool_parses_its_arguments(monkeypatch, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("eval_poses", os.path.join(REPO, "tools", "eval_poses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.RandomState(0)
    for name in ("pred", "gt"):
        os.makedirs(tmp_path / name)
        np.save(tmp_path / name / "poses.npy", rng.normal(0, 1, (3, 2, 72)))
        np.save(tmp_path / name / "normalize_trans.npy", rng.normal(0, 1, (3, 2, 3)))
        np.save(tmp_path / name / "mean_shape.npy", rng.normal(0, 1, (2, 10)))
    np.save(tmp_path / "gt" / "gender.npy", np.array(["male", "female"]))
    seen = {}

    class Server:
        faces = FACES
    monkeypatch.setattr(hip, "require_device", lambda: None)
    monkeypatch.setattr(mod, "make_servers", lambda g, b: seen.update(genders=g, betas=b) or [Server(), Server()])
    monkeypatch.setattr(PM, "pose_sequence", lambda s, p: seen.update(posed=p) or ("V", "J"))
    monkeypatch.setattr(PM, "contacts_from_bodies", lambda v, f, t: seen.update(cfb=(v, f, t)) or "C")
    monkeypatch.setattr(PM, "pose_metrics", lambda *a, **k: seen.update(a=a, k=k) or {"mean_mpjpe": 1.5, "mpjpe": np.array([[1.0, 2.0]])})
    out = mod.main([str(tmp_path / "pred"), str(tmp_path / "gt"), "--scale", "100"])
    assert out["mean_mpjpe"] == 1.5 and seen["genders"] == ["male", "female"] and seen["betas"].shape == (2, 10)
    pred, gt = seen["a"]
    assert pred.shape == gt.shape == (3, 2, 86) and pred.dtype == np.float32 and (pred[..., 0] == 1).all()
    assert np.array_equal(gt[..., 4:76], np.load(tmp_path / "gt" / "poses.npy").astype(np.float32))
    assert np.array_equal(gt[1, :, 76:], np.load(tmp_path / "gt" / "mean_shape.npy").astype(np.float32))
    assert seen["k"]["unit_scale"] == 100.0 and seen["k"]["contacts"] is None and seen["k"]["depth_threshold"] == 0.15 and "posed" not in seen
    mod.main([str(tmp_path / "pred"), str(tmp_path / "gt"), "--gender", "neutral", "--contact-threshold", "0.02", "--smpl-scale", "1.1",
              "--depth-threshold", "0.2"])
    assert seen["genders"] == ["neutral", "neutral"] and seen["cfb"] == ("V", FACES, 0.02) and seen["k"]["contacts"] == "C"
    assert seen["a"][1] == {"verts": "V", "joints": "J"} and np.allclose(seen["a"][0][..., 0], 1.1) and seen["k"]["depth_threshold"] == 0.2
    assert mod.jsonable({"a": np.array([1.0, 2.0]), "b": 3}) == {"a": [1.0, 2.0], "b": 3}
    with pytest.raises(ValueError, match="--gender"):
        mod.main([str(tmp_path / "pred"), str(tmp_path / "gt"), "--gender", "a", "b", "c"])
