"""The pose-metric kernels and multiply_amd.pose_metrics on the device against the float64 restatement
(tests/pose_metrics_reference.py); bounds: tests/tolerances_pose_metrics.py."""
import numpy as np
import pytest
import torch

from multiply_amd import hip, pose_metrics as PM
from oracle import multiply_oracle as O
from tests import mesh_metrics_reference as MR
from tests import pose_metrics_reference as R
from tests import tolerances_mesh_metrics as MTOL
from tests import tolerances_pose_metrics as TOL
from tests.test_pose_metrics_cpu import rotation
from tests.util import t32

pytestmark = pytest.mark.gpu

KINDS = ("random", "mirrored", "coplanar", "nearplanar")


def item(kind, n, seed):
    """(pred, gt) (n, 3) float32 of one kind"""
    rng = np.random.RandomState(seed)
    gt = rng.normal(0, 1, (n, 3)) * np.array([1.0, 0.7, 0.4]) + np.array([0.3, -0.2, 2.0])
    rigid = lambda x: x @ rotation(rng.normal(0, 1, 3), rng.uniform(0.3, 2.5)).T + rng.normal(0, 0.5, 3)
    if kind == "random":
        pred = 1.1 * rigid(gt + rng.normal(0, 0.05, (n, 3)))
    elif kind == "mirrored":
        pred = gt * np.array([-1.0, 1.0, 1.0])
    elif kind == "coplanar":
        gt[:, 2] = 0.0
        pred = rigid(gt)
    else:
        gt[:, 2] = 2.0 + 1e-3 * np.abs(gt).max() * rng.uniform(-0.5, 0.5, n)       # z-spread 1e-3 of the extent
        pred = rigid(gt) + rng.normal(0, 1e-3, (n, 3))
    return pred.astype(np.float32), gt.astype(np.float32)


def launch(pred, gt, roots=True):
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    r = (p[:, 0].contiguous(), g[:, 0].contiguous()) if roots else ()
    return hip.pose_errors(p, g, *r).cpu().numpy()


def compare(pred, gt, got, tag):
    want = R.pose_errors(pred, gt, pred[:, 0], gt[:, 0])
    worst = 0.0
    for m in range(len(pred)):
        M = TOL.coordinate_scale(pred[m], gt[m])
        rel = np.abs(got[m, :2] - want[m, :2]) / np.maximum(np.abs(want[m, :2]), 1e-300)
        pa = abs(got[m, 2] - want[m, 2]) / M
        worst = max(worst, pa)
        print(f"[pose_errors vs float64] {tag} item {m}: plain {rel[0]:.2e} aligned {rel[1]:.2e} (relative)  "
              f"procrustes {pa:.3e} of M = {M:.2f} (value {want[m, 2]:.3e})")
        assert got[m, 3] == want[m, 3] == 0
        assert rel[0] <= TOL.SUMS and rel[1] <= TOL.SUMS, (tag, m)
    return worst


@pytest.mark.parametrize("n", [3, 24, 257, 6890])
@pytest.mark.parametrize("kind", KINDS)
def test_pose_errors_against_the_restatement(kind, n):
    pred, gt = item(kind, n, seed=n + KINDS.index(kind))
    worst = compare(pred[None], gt[None], launch(pred[None], gt[None]), f"{kind} n {n} M 1")
    assert worst <= TOL.PROCRUSTES, (kind, n, worst)


@pytest.mark.parametrize("n", [3, 24, 257, 6890])
def test_pose_errors_of_five_items(n):
    items = [item(k, n, seed=100 + n + i) for i, k in enumerate(KINDS + ("random",))]
    pred, gt = np.stack([a for a, _ in items]), np.stack([b for _, b in items])
    got = launch(pred, gt)
    worst = compare(pred, gt, got, f"all kinds n {n} M 5")
    assert worst <= TOL.PROCRUSTES, (n, worst)
    for m in range(5):                                              # an item's values do not depend on its launch
        assert np.array_equal(launch(pred[m:m + 1], gt[m:m + 1])[0], got[m])
    assert np.array_equal(launch(pred, gt), got)
    no_roots = launch(pred, gt, roots=False)
    assert np.isnan(no_roots[:, 1]).all() and np.array_equal(no_roots[:, [0, 2, 3]], got[:, [0, 2, 3]])


def test_left_out_items_are_nan_counted_and_disturb_nobody():
    items = [item("random", 24, seed=i) for i in range(4)]
    pred, gt = np.stack([a for a, _ in items]), np.stack([b for _, b in items])
    clean = launch(pred, gt)
    pred[1, 7, 2] = np.nan
    pred[2] = pred[2, :1]                                           # every predicted point coincides
    got = launch(pred, gt)
    want = R.pose_errors(pred, gt, pred[:, 0], gt[:, 0])
    assert got[:, 3].tolist() == want[:, 3].tolist() == [0, 1, 2, 0]
    assert np.isnan(got[1, :3]).all() and np.isnan(got[2, 2])
    assert np.abs(got[2, :2] - want[2, :2]).max() <= TOL.SUMS * np.abs(want[2, :2]).max()
    assert np.array_equal(got[[0, 3]], clean[[0, 3]])
    gt[0, 3, 0] = np.inf                                            # the ground truth and the roots count too
    assert launch(pred, gt)[0, 3] == 1
    pred2, gt2 = np.stack([a for a, _ in items]), np.stack([b for _, b in items])
    p, g = torch.from_numpy(pred2).cuda(), torch.from_numpy(gt2).cuda()
    bad_root = g[:, 0].clone()
    bad_root[3, 1] = float("nan")
    out = hip.pose_errors(p, g, p[:, 0].contiguous(), bad_root).cpu().numpy()
    assert out[:, 3].tolist() == [0, 0, 0, 1] and np.isnan(out[3, :3]).all()
    # through the public call: NaN in the per-item arrays, counted, left out of the means
    d = lambda x: {"joints": torch.from_numpy(x.reshape(2, 2, 24, 3))}
    res = PM.pose_metrics(d(pred), d(np.stack([b for _, b in items])))
    assert res["n_left_out_joints"] == 1 and res["n_degenerate_joints"] == 1 and res["n_items"] == 4
    assert np.isnan(res["mpjpe"][0, 1]) and np.isnan(res["pa_mpjpe"][1, 0]) and np.isfinite(res["mpjpe"][1, 0])
    assert abs(res["mean_mpjpe"] - np.nanmean(res["mpjpe"])) <= 1e-15 and np.isfinite(res["mean_pa_mpjpe"])


# ------------------------------------------------------------------------------------------------ bodies
@pytest.fixture(scope="module")
def scene(smpl_tables):
    """F = 4, P = 2: ground-truth parameters, a perturbed prediction, the servers, and the ORACLE's bodies of both"""
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_scene
    F, P = 4, 2
    rng = np.random.RandomState(11)
    base = make_scene(P, seed=0, H=16, W=16)["smpl_params"][0]
    gt = np.repeat(base[None], F, 0).astype(np.float32)
    gt[:, :, 4:76] += rng.normal(0, 0.05, (F, P, 72)).astype(np.float32)
    gt[:, :, 1:4] += rng.normal(0, 0.05, (F, P, 3)).astype(np.float32)
    pred = gt.copy()
    pred[:, :, 4:76] += rng.normal(0, 0.02, (F, P, 72)).astype(np.float32)
    pred[:, :, 1:4] += rng.normal(0, 0.01, (F, P, 3)).astype(np.float32)
    servers = [SMPLServer(gender="male", betas=base[p, 76:], smpl_tables=smpl_tables) for p in range(P)]
    refs = [O.SMPLServerOracle(smpl_tables, base[p, 76:]) for p in range(P)]

    def bodies(prm):
        v, j = np.zeros((F, P, 6890, 3), np.float32), np.zeros((F, P, 24, 3), np.float32)
        for f in range(F):
            for p in range(P):
                r = t32(prm[f, p])
                o = refs[p].forward(r[0], r[1:4], r[4:76], r[76:])
                v[f, p], j[f, p] = o["smpl_verts"].numpy(), o["smpl_jnts"].numpy()
        return {"verts": v, "joints": j}
    faces = np.asarray(servers[0].faces)
    c = random_contacts(np.random.RandomState(3), F, P, 6890, faces.shape[0], 50, empty_frame=1)
    return dict(F=F, P=P, gt=gt, pred=pred, servers=servers, oracle_gt=bodies(gt), oracle_pred=bodies(pred), faces=faces, contacts=c)


def random_contacts(rng, F, P, V, n_faces, m, empty_frame):
    frame = rng.choice([f for f in range(F) if f != empty_frame], m)
    a = rng.randint(0, P, m)
    return dict(frame=frame.astype(np.int32), person_a=a.astype(np.int32), vertex=rng.randint(0, V, m).astype(np.int32),
                person_b=((a + 1 + rng.randint(0, P - 1, m)) % P).astype(np.int32), face=rng.randint(0, n_faces, m).astype(np.int32),
                bary=rng.dirichlet([1, 1, 1], m).astype(np.float32))


def test_contact_distance_against_the_restatement(scene):
    F, P = 3, scene["P"]
    verts = torch.from_numpy(scene["oracle_gt"]["verts"][:F]).cuda()
    faces = scene["faces"]
    c = random_contacts(np.random.RandomState(4), F, P, 6890, faces.shape[0], 50, empty_frame=1)
    order = np.argsort(c["frame"], kind="stable")
    corr = np.stack([c[k][order] for k in ("frame", "person_a", "vertex", "person_b", "face")], 1).astype(np.int32)
    start = np.searchsorted(c["frame"][order], np.arange(F + 1)).astype(np.int32)
    args = (verts, torch.from_numpy(faces.astype(np.int32)).cuda(), torch.from_numpy(corr).cuda(), torch.from_numpy(c["bary"][order]).cuda(),
            torch.from_numpy(start).cuda())
    got = hip.contact_distance(*args).cpu().numpy()
    mean, per, cnt = R.contact_distance(verts.cpu().numpy(), faces, c)
    rel = max(abs(got[0] - mean) / mean, np.nanmax(np.abs(got[2:2 + F] - per) / per))
    print(f"[contact distance vs float64] mean {mean:.4f}: relative error {rel:.2e}; counts {got[2 + F:].tolist()}")
    assert rel <= TOL.SUMS
    assert np.isnan(got[3]) and got[2 + F:].tolist() == cnt.tolist() and cnt[1] == 0 and got[1] == 50
    assert np.array_equal(hip.contact_distance(*args).cpu().numpy(), got, equal_nan=True)
    empty = hip.contact_distance(verts, args[1], args[2][:0], args[3][:0], torch.zeros(F + 1, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.isnan(empty[0]) and empty[1] == 0 and np.isnan(empty[2:2 + F]).all() and not empty[2 + F:].any()


def test_contacts_from_bodies(scene):
    """two posed bodies moved together until they overlap, against a sparse set of one body's faces"""
    v = scene["oracle_gt"]["verts"][:1].copy()
    v[0, 1] += (v[0, 0].mean(0) - v[0, 1].mean(0)) + np.array([0.12, 0.0, 0.03], np.float32)
    faces = scene["faces"][::92]
    D = {(p, q): np.sqrt(np.nanmin(MR.all_d2(v[0, p], v[0, q][faces]), axis=1)) for p, q in ((0, 1), (1, 0))}
    M = MTOL.coordinate_scale(v)
    delta = MTOL.delta(M)
    alld = np.sort(np.concatenate(list(D.values())))
    k = np.searchsorted(alld, 0.02)
    gaps = alld[k - 40:k + 40]
    g = int(np.argmax(np.diff(gaps)))
    threshold = float(0.5 * (gaps[g] + gaps[g + 1]))               # the middle of the widest gap between distances near 0.02
    margin = np.abs(alld - threshold).min()
    print(f"[contacts] M {M:.2f} delta {delta:.2e} threshold {threshold:.6f} margin {margin:.2e}")
    assert margin > delta                                           # no vertex's float64 distance lies within delta of the threshold
    c = PM.contacts_from_bodies(torch.from_numpy(v), faces, threshold)
    m = c["frame"].shape[0]
    assert m > 50 and not c["frame"].any() and all(c[k].shape == (m,) for k in ("person_a", "vertex", "person_b", "face"))
    for (p, q), d in D.items():
        sel = (c["person_a"] == p) & (c["person_b"] == q)
        assert sorted(c["vertex"][sel].tolist()) == np.nonzero(d <= threshold)[0].tolist(), (p, q)
        vert, face = c["vertex"][sel], c["face"][sel]
        tri = v[0, q][faces[face]]
        d2f, qf = MR.closest_points_paired(v[0, p][vert], tri)     # the float64 closest point ON THE REPORTED FACE
        e_f = (np.sqrt(d2f) - d[vert]).max()
        point = (c["bary"][sel].astype(np.float64)[:, :, None] * tri.astype(np.float64)).sum(1)
        e_q = np.linalg.norm(point - qf, axis=1).max()
        # the reference's own closest point (over all faces): where its face is the reported one the two points must agree as
        # well.  Where the faces differ -- two faces as near as each other to within face_membership, e.g. across an edge -- their
        # closest points may lie apart, and the point is held to the reported face alone (above), the face to its distance.
        _, f64, q64 = MR.closest(v[0, p][vert], v[0, q][faces])
        same = f64 == face
        e_g = np.linalg.norm(point - q64, axis=1)[same].max()
        # what taking the barycentrics from the QUERY's fp32 closest point would give (a figure, not a check: DESIGN 6i)
        _, fk, qk = hip.mesh_closest(torch.from_numpy(v[0, p][vert]).cuda(), torch.from_numpy(v[0, q][faces]).cuda())
        assert np.array_equal(fk.cpu().numpy(), face)
        e_k = np.linalg.norm(qk.cpu().numpy().astype(np.float64) - qf, axis=1).max()
        print(f"[contacts] pair {(p, q)}: {sel.sum()} contacts, face {e_f:.2e} (<= {MTOL.face_membership(M):.2e}), point {e_q:.2e} on the "
              f"reported face, {e_g:.2e} against the reference's point on the {same.sum()} with the same face (<= {delta:.2e}); "
              f"the query's own fp32 point: {e_k:.2e}")
        assert e_f <= MTOL.face_membership(M) and e_q <= delta and e_g <= delta and same.mean() > 0.5
    assert (c["bary"] >= 0).all() and np.abs(c["bary"].sum(1) - 1).max() <= 2e-7
    # on the bodies they were built from, the contact distance is the distance to the surface: at most the threshold
    res = PM.pose_metrics({"verts": torch.from_numpy(v)}, {"verts": torch.from_numpy(v)}, contacts=c, faces=faces)
    assert res["cd"] == res["cd_gt"] <= threshold and res["n_contacts"] == m


VIEW = np.array([[0.8, 0.0, 0.6, 0.1], [0.0, 1.0, 0.0, -0.2], [-0.6, 0.0, 0.8, 2.5]], np.float32)


def test_pose_metrics_end_to_end(scene):
    kw = dict(root=0, unit_scale=100.0, contacts=scene["contacts"], faces=scene["faces"], view=VIEW, depth_threshold=1.0)
    got = PM.pose_metrics(scene["pred"], scene["gt"], servers=scene["servers"], **kw)
    want = R.metrics(scene["oracle_pred"], scene["oracle_gt"], **kw)
    M = TOL.coordinate_scale(scene["oracle_pred"]["verts"], scene["oracle_gt"]["verts"])
    for key in PM.DISTANCE_KEYS:
        assert got[key].shape == (scene["F"], scene["P"])
        e = np.abs(got[key] - want[key])
        bound = np.array([[TOL.end_to_end(key, v, M, 100.0) for v in row] for row in want[key]])
        print(f"[pose_metrics vs float64 on the oracle's bodies] {key}: mean {want['mean_' + key]:.4f} cm, worst error {e.max():.2e} (bound {bound.min():.2e})")
        assert (e <= bound).all(), key
        assert abs(got["mean_" + key] - want["mean_" + key]) <= bound.max()
    for key in ("cd", "cd_gt"):
        assert abs(got[key] - want[key]) <= TOL.end_to_end(key, want[key], M, 100.0)
        ok = ~np.isnan(want[key + "_per_frame"])
        assert (np.isnan(got[key + "_per_frame"]) == ~ok).all()
        assert (np.abs(got[key + "_per_frame"] - want[key + "_per_frame"])[ok] <= TOL.end_to_end(key, np.nanmax(want[key + "_per_frame"]), M, 100.0)).all()
    assert got["n_contacts"] == 50 and got["n_contacts_per_frame"].tolist() == want["n_contacts_per_frame"].tolist() and got["n_contacts_per_frame"][1] == 0
    zp, zg = (R.depths(scene[k]["joints"][:, :, 0], VIEW) for k in ("oracle_pred", "oracle_gt"))
    assert min(R.relations(zp, 1.0, 100.0)[1].min(), R.relations(zg, 1.0, 100.0)[1].min()) > 100.0 * 10 * TOL.POSE_POINTS
    assert got["pcdr"] == want["pcdr"] and got["n_depth_pairs"] == want["n_depth_pairs"] == scene["F"]
    assert got["n_left_out_joints"] == got["n_left_out_verts"] == got["n_degenerate_verts"] == 0 and got["n_items"] == 8


def test_pose_metrics_of_equal_sequences_is_exactly_zero(scene):
    got = PM.pose_metrics(scene["gt"], scene["gt"], servers=scene["servers"], contacts=scene["contacts"], faces=scene["faces"])
    for key in PM.DISTANCE_KEYS:
        assert (got[key] == 0.0).all() and got["mean_" + key] == 0.0, key
    assert got["pcdr"] == 1.0 and got["cd"] == got["cd_gt"]
    only_joints = PM.pose_metrics(scene["gt"], {"joints": scene["oracle_gt"]["joints"]}, servers=scene["servers"])
    assert "mve" not in only_joints and only_joints["mean_mpjpe"] <= 100 * TOL.POSE_POINTS      # ground truth as joints alone
    reg = torch.zeros(3, 6890)
    reg[0, 10] = reg[1, 20] = reg[2, 30] = 1.0
    picked = PM.pose_metrics(scene["pred"], scene["gt"], servers=scene["servers"], joint_regressor=reg, root=1)
    plain = PM.pose_metrics(scene["pred"], scene["gt"], servers=scene["servers"])
    assert picked["mpjpe"].shape == (4, 2) and picked["mean_mpjpe_global"] != plain["mean_mpjpe_global"]
    assert np.array_equal(picked["mve_global"], plain["mve_global"])


def test_pcdr_counts_are_exact():
    """three persons, depths built so that every | |d| - threshold | >= 1e-3 (fp32 depths are good to ~1e-6)"""
    from tests.test_pose_metrics_cpu import PCDR, Z_GT, Z_PRED
    thr = 0.15
    for z in (Z_GT, Z_PRED):
        assert R.relations(z, thr)[1].min() >= 1e-3
    rot = rotation([0.2, 1.0, -0.3], 0.7)
    view = np.concatenate([rot, np.array([[0.3], [-0.1], [0.4]])], 1)

    def joints(z, with_view):
        cam = np.stack([np.full(z.shape, 0.3), np.full(z.shape, -0.7), z], -1)           # camera coordinates, depth = z
        world = (cam - view[:, 3]) @ rot if with_view else cam                           # camera = rot world + t
        return {"joints": world[:, :, None, :].astype(np.float32)}
    for with_view in (False, True):
        got = PM.pose_metrics(joints(Z_PRED, with_view), joints(Z_GT, with_view), view=view.astype(np.float32) if with_view else None,
                              depth_threshold=thr)
        assert got["pcdr"] == PCDR and got["n_depth_pairs"] == 6 and got["pcdr_per_frame"].tolist() == [2 / 3, 1 / 3]
    scaled = PM.pose_metrics(joints(Z_PRED, False), joints(Z_GT, False), unit_scale=100.0, depth_threshold=15.0)
    assert scaled["pcdr"] == PCDR
    one = PM.pose_metrics({"joints": joints(Z_PRED, False)["joints"][:, :1]}, {"joints": joints(Z_GT, False)["joints"][:, :1]})
    assert np.isnan(one["pcdr"]) and one["n_depth_pairs"] == 0 and np.isnan(one["pcdr_per_frame"]).all()
