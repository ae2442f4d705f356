"""Host side of the keypoint fit (multiply_amd/keypoint_fit.py) and the float64 restatement the device tests compare against
(tests/keypoint_fit_reference.py): the restatement is pinned on the reference's own rot6D (a recorded fixture), on hand-computed
GMoF / projection values and on torch.optim.Adam before tests/test_keypoint_fit_gpu.py relies on it."""
import os
import warnings

import numpy as np
import pytest
import torch

from multiply_amd import keypoint_fit as KF
from tests import keypoint_fit_cases as C
from tests import keypoint_fit_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoint_fit_golden.npz")


def test_rot6d_equals_the_references_axis_to_rot6d():
    """the fixture records rotation.py::axis_to_rot6D (through a quaternion, float32) on a zero rotation, rotations near pi and
    random ones; the restatement takes the first two columns of Rodrigues' matrix.  Both are float32-exact to a few ulp of 1."""
    g = np.load(GOLDEN)
    axis = g["axis"]
    assert (axis[0] == 0).all() and abs(np.linalg.norm(axis[1]) - np.pi) < 2e-3 and abs(np.linalg.norm(axis[2]) - np.pi) < 2e-3
    want = g["rot6d"].reshape(24, 6).astype(np.float64)
    got = R.rot6d(torch.from_numpy(axis).double()).numpy()
    assert np.abs(got - want).max() < 8 * np.finfo(np.float32).eps          # the fixture's own float32 rounding (measured 2.4e-7)
    np.testing.assert_array_equal(got[0], [1, 0, 0, 1, 0, 0])               # zero rotation: the identity's first two columns


def test_gmof_and_projection_on_hand_computed_values():
    r = torch.tensor([0.0, 100.0, -300.0, 1.0], dtype=torch.float64)
    np.testing.assert_allclose(R.gmof(r, 100.0).numpy(), [0.0, 5000.0, 9000.0, 1e4 / 10001.0], rtol=1e-15)
    # x_c = E [x; 1] with E = [I | (0, 0, 1)]: (1, 2, 4) -> (1, 2, 5); u = 500 * 1 / 5 + 10 = 110, v = 250 * 2 / 5 + 20 = 120
    cam = torch.tensor([500.0, 250.0, 10.0, 20.0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1], dtype=torch.float64)
    uv, z = R.project(torch.tensor([[1.0, 2.0, 4.0]], dtype=torch.float64), cam)
    np.testing.assert_allclose(uv.numpy(), [[110.0, 120.0]], rtol=1e-15)
    assert float(z) == 5.0
    rows = KF.camera_rows({"intrinsics": [[500, 0, 10], [0, 250, 20], [0, 0, 1]], "extrinsic": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1]]}, 2)
    np.testing.assert_array_equal(rows.numpy(), np.tile(cam.numpy().astype(np.float32), (2, 1)))
    np.testing.assert_array_equal(KF.camera_rows({"fx": 1, "fy": 2, "cx": 3, "cy": 4}, 1).numpy()[0, 4:], np.eye(4)[:3].reshape(-1))


def test_restatement_total_is_the_references_loss(smpl_tables):
    """joints_2d_loss (a mean over K x 2 of squared weights times GMoF) and the temporal term, spelled as in loss.py, on one row"""
    T = R.tables64(smpl_tables)
    cs = C.objective_case(T, "coco25-shaped")
    kmap, n = cs["kmap"], 1
    conf = torch.rand(kmap.K, generator=torch.Generator().manual_seed(2)).double()
    c = KF.keypoint_weights(conf, kmap, 0.6)
    terms, proj, _ = R.objective(T, kmap, cs["params"][n], cs["targets"][n], c, cs["cam"][n], cs["prev"][n])
    conf_t = torch.where(conf < 0.6, torch.zeros_like(conf), conf)
    jw = torch.ones(25, dtype=torch.float64)
    jw[[1, 9, 12]] = 0
    j2d = torch.mean((conf_t * jw).unsqueeze(-1) ** 2 * R.gmof(cs["targets"][n] - proj, 100.0))
    prev, p = cs["prev"][n], cs["params"][n]
    temporal = torch.mean((R.rot6d(prev[3:75]) - R.rot6d(p[3:75])) ** 2) * 5 + torch.mean((prev[:3] - p[:3]) ** 2)
    np.testing.assert_allclose(float(terms[0]), float(j2d), rtol=1e-13)
    np.testing.assert_allclose(float(terms[1]), float(temporal), rtol=1e-13)
    np.testing.assert_allclose(float(terms[2]), 1e-2 * float(j2d) + 6.0 * float(temporal), rtol=1e-13)


def test_reduced_tables_give_the_full_bodys_keypoints_and_gradient(smpl_tables):
    T = R.tables64(smpl_tables)
    cs = C.objective_case(T, "mixed")
    Tr, kr = cs["reduced"]
    a = R.objective_and_grad(T, cs["kmap"], cs["params"][2], cs["targets"][2], cs["c"][2], cs["cam"][2], cs["prev"][2])
    b = R.objective_and_grad(Tr, kr, cs["params"][2], cs["targets"][2], cs["c"][2], cs["cam"][2], cs["prev"][2])
    for x, y in zip(a[:3], b[:3]):
        assert float((x - y).abs().max()) <= 1e-11 * max(1.0, float(x.abs().max()))


def test_adam_step_equals_torch_optim_adam_on_a_quadratic():
    g = torch.Generator().manual_seed(4)
    A = torch.randn(85, 85, generator=g).double()
    A = A @ A.T / 85 + torch.eye(85).double()
    b = torch.randn(85, generator=g).double()
    x0 = torch.randn(85, generator=g).double()
    lrs = (1e-3, 2e-3, 5e-4)
    parts = [x0[0:3].clone().requires_grad_(True), x0[3:75].clone().requires_grad_(True), x0[75:].clone().requires_grad_(True)]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(parts, lrs)], lr=2e-3, betas=(0.9, 0.999))
    p, m, v, lr = x0.clone(), torch.zeros(85).double(), torch.zeros(85).double(), R.lr_row(lrs)
    for it in range(30):
        opt.zero_grad()
        x = torch.cat(parts)
        (0.5 * x @ A @ x - b @ x).backward()
        opt.step()
        p, m, v = R.adam_step(p, A @ p - b, m, v, it + 1, lr)
        assert float((torch.cat(parts).detach() - p).abs().max()) < 1e-14


# ---------------------------------------------------------------------------------------------- KeypointMap
def test_keypoint_map_validation():
    ok = KF.KeypointMap([0, 1, 3], [3, 24, 25], [1.0, 0.5, 0.5], support=[7, 9])
    assert (ok.K, ok.S) == (2, 2) and ok.row_kinds() == ["joint", "regressor"]
    np.testing.assert_array_equal(ok.dense(), [[0] * 3 + [1] + [0] * 22, [0] * 24 + [0.5, 0.5]])
    for bad, match in (
            (dict(ptr=[0, 2, 1], idx=[0], w=[1.0]), "non-decreasing"),
            (dict(ptr=[1, 2], idx=[0, 1], w=[1.0, 1.0]), "starts at 0"),
            (dict(ptr=[0, 1], idx=[24], w=[1.0]), r"\[0, 24\)"),
            (dict(ptr=[0, 1], idx=[24], w=[1.0], support=[6890]), "unique vertex ids"),
            (dict(ptr=[0, 1], idx=[24], w=[1.0], support=[5, 5]), "unique"),
            (dict(ptr=[0, 1], idx=[0], w=[float("nan")]), "finite"),
            (dict(ptr=[0, 1], idx=[0.5], w=[1.0]), "integers"),
            (dict(ptr=[0, 2], idx=[0], w=[1.0]), r"expected \(2,\)"),
            (dict(ptr=np.arange(KF.MAX_K + 2), idx=np.zeros(KF.MAX_K + 1, int), w=np.ones(KF.MAX_K + 1)), "MP_KP_MAX_K"),
            (dict(ptr=[0, 1], idx=[0], w=[1.0], support=np.arange(KF.MAX_S + 1)), "MP_KP_MAX_S"),
            (dict(ptr=[0, 1], idx=[0], w=[1.0], joint_weights=[1.0, 1.0]), "joint_weights")):
        with pytest.raises(ValueError, match=match):
            KF.KeypointMap(**bad)
    with pytest.raises(ValueError, match="joint id 24"):
        KF.KeypointMap.from_joints([24])
    with pytest.raises(ValueError, match="vertex id 6890"):
        KF.KeypointMap.from_vertices([6890])
    with pytest.raises(ValueError, match=r"\(R, 6890\)"):
        KF.KeypointMap.from_regressor(np.zeros((2, 10)))


def test_transposed_map_is_the_same_matrix():
    for name, m in C.maps().items():
        tp, tk, tw = m.transposed()
        D = np.zeros((m.K, 24 + m.S))
        for i in range(24 + m.S):
            assert (np.diff(tk[tp[i]:tp[i + 1]]) >= 0).all()
            for e in range(tp[i], tp[i + 1]):
                D[tk[e], i] += tw[e]
        np.testing.assert_array_equal(D, m.dense(), err_msg=name)
    mixed = C.maps()["mixed"]
    assert mixed.row_kinds() == ["joint", "vertex", "regressor", "regressor", "joint"] and mixed.S == 5      # one vertex shared


def test_coco_builders_row_kinds():
    ex = C.extra_regressor()
    m25 = KF.KeypointMap.coco25(ex)
    assert m25.K == 25 and m25.row_kinds() == ["vertex"] + ["joint"] * 14 + ["vertex"] * 10
    assert [r[1] for r in m25.rows()[:9]] == [332, 12, 17, 19, 21, 16, 18, 20, 0]
    assert [r[1] for r in m25.rows()[15:]] == [6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787]
    assert sorted(np.nonzero(m25.joint_weights == 0)[0].tolist()) == [1, 9, 12]
    m17 = KF.KeypointMap.coco17(ex)
    assert m17.row_kinds() == ["vertex"] * 5 + ["joint"] * 6 + ["regressor"] * 2 + ["joint"] * 4
    # keypoints 11, 12 = joints 46, 45 of the 54 = rows 1, 0 of the extra regressor
    D = m17.dense()
    for k, r in ((11, 1), (12, 0)):
        row = np.zeros(6890)
        row[m17.support] = D[k, 24:]
        np.testing.assert_allclose(row, ex[r], rtol=1e-7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        bare = KF.KeypointMap.coco17()
    assert len(w) == 1 and "J_regressor_extra.npy" in str(w[0].message) and "[11, 12]" in str(w[0].message)
    assert bare.row_kinds()[11:13] == ["empty", "empty"] and (bare.joint_weights[11:13] == 0).all() and bare.notes
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        KF.KeypointMap.coco25()                      # coco25 needs no extra row: no message
    with pytest.raises(ValueError, match=r"\(9, 6890\)"):
        KF.KeypointMap.coco17(np.zeros((8, 6890)))


def test_keypoint_weights_threshold_ignored_joints_and_two_sets():
    m25 = KF.KeypointMap.coco25()
    conf = torch.full((2, 25), 0.8)
    conf[0, 4] = 0.59
    conf[1, 7] = 0.6
    c = KF.keypoint_weights(conf, m25, 0.6)
    want = torch.full((2, 25), 0.8 ** 2 / 50)
    want[:, [1, 9, 12]] = 0
    want[0, 4] = 0
    want[1, 7] = 0.6 ** 2 / 50
    np.testing.assert_allclose(c.numpy(), want.numpy(), rtol=1e-6)
    both = m25.concat(KF.KeypointMap.from_joints([7, 8], joint_weights=[1.0, 0.5]))
    assert both.K == 27 and both.sets == [(0, 25), (25, 27)] and both.S == m25.S
    conf2 = torch.cat([conf, torch.tensor([[0.5, 0.3], [0.39, 0.9]])], 1)
    c2 = KF.keypoint_weights(conf2, both, (0.6, 0.4))
    np.testing.assert_allclose(c2[:, :25].numpy(), want.numpy(), rtol=1e-6)
    np.testing.assert_allclose(c2[:, 25:].numpy(), [[0.5 ** 2 / 4, 0.0], [0.0, (0.9 * 0.5) ** 2 / 4]], rtol=1e-6)
    with pytest.raises(ValueError, match=r"\(\.\.\., 25\)"):
        KF.keypoint_weights(torch.zeros(2, 24), m25)
    with pytest.raises(ValueError, match="one per keypoint set"):
        KF.keypoint_weights(conf2, both, (0.6, 0.4, 0.1))


# ---------------------------------------------------------------------------------------------- sequencing
def test_sequence_loop_start_values_targets_and_copied_frames():
    F, P = 4, 3
    init = torch.arange(F * P * 85, dtype=torch.float64).reshape(F, P, 85)
    tracked = torch.zeros(F, P, dtype=torch.bool)
    tracked[2, 1] = tracked[3, 0] = tracked[0, 2] = True      # (a tracked pair in frame 0 has no previous frame: ignored)
    calls = []

    def fit(f, start, prev):
        calls.append((f, start.clone(), prev.clone()))
        return start + 0.5

    res, prevs = KF.sequence_loop(init, tracked, (1,), fit)
    assert [c[0] for c in calls] == [0, 2, 3]
    np.testing.assert_array_equal(calls[0][1], init[0])
    np.testing.assert_array_equal(calls[0][2], init[0][:, :75])                  # frame 0: its own initial values as target
    np.testing.assert_array_equal(res[0], init[0] + 0.5)
    np.testing.assert_array_equal(res[1], torch.cat([res[0][:, :75], init[1][:, 75:]], 1))     # copied frame, own betas
    want2 = init[2].clone()
    want2[1] = res[1][1]
    np.testing.assert_array_equal(calls[1][1], want2)                            # tracked pair starts from the previous result
    np.testing.assert_array_equal(calls[1][2], res[1][:, :75])
    want3 = init[3].clone()
    want3[0] = res[2][0]
    np.testing.assert_array_equal(calls[2][1], want3)
    np.testing.assert_array_equal(prevs[3], res[2][:, :75])
    np.testing.assert_array_equal(prevs[1], res[0][:, :75])


def test_refine_sequence_rejects_bad_shapes():
    kmap = KF.KeypointMap.from_joints([0, 1])
    good = dict(pose=torch.zeros(2, 1, 72), trans=torch.zeros(2, 1, 3), shape=torch.zeros(2, 1, 10))
    kp = torch.zeros(2, 1, 2, 3)
    cam = {"fx": 1, "fy": 1, "cx": 0, "cy": 0}
    for init, kps, kw, match in (
            (dict(good, pose=torch.zeros(2, 1, 71)), kp, {}, r"\(2, 1, 71\)"),
            (dict(good, trans=torch.zeros(2, 2, 3)), kp, {}, r"\(2, 2, 3\)"),
            (good, torch.zeros(2, 1, 3, 3), {}, r"\(2, 1, 3, 3\)"),
            (good, kp.long(), {}, "int64"),
            (good, kp, dict(tracking=[(2, 0)]), r"\(2, 0\)"),
            (good, kp, dict(interpolate_frames=[5]), "frame 5"),
            ({"pose": torch.zeros(2, 1, 72)}, kp, {}, "dict with")):
        with pytest.raises(ValueError, match=match):
            KF.refine_sequence([None], init, kps, cam, kmap, **kw)
    with pytest.raises(ValueError, match=r"\(3, 5\)"):
        KF.camera_rows(torch.zeros(3, 5), 3)


def test_float64_loop_at_least_halves_the_recovery_error():
    """the perturbation of the recovery sequence (tests/keypoint_fit_cases.py) is one the float64 loop recovers from: the device
    test asks the kernel for the same fall"""
    ref = C.recovery_reference()
    print(f"recovery: mean reprojection error {ref['before']:.3f} px -> {ref['after']:.3f} px")
    assert ref["before"] > 5.0 and ref["after"] <= 0.5 * ref["before"]
    res, cs = ref["results"], C.recovery_case()
    np.testing.assert_array_equal(res[1][:, :75], res[0][:, :75])               # the copied frame
    np.testing.assert_array_equal(res[1][:, 75:], cs["init"][1][:, 75:].double())
    np.testing.assert_array_equal(ref["prev"][2], res[1][:, :75])


def test_second_keypoint_set_is_one_concatenated_map():
    """refine_sequence's host preparation: two detectors' keypoints become one map, each set with its own K_set and threshold"""
    first, second = KF.KeypointMap.from_joints([0, 1, 2, 3]), KF.KeypointMap.from_joints([7, 8], joint_weights=[1.0, 0.0])
    init = dict(pose=torch.zeros(2, 1, 72), trans=torch.zeros(2, 1, 3), shape=torch.zeros(2, 1, 10))
    kp1 = torch.rand(2, 1, 4, 3, generator=torch.Generator().manual_seed(0))
    kp1[..., 2] = torch.tensor([0.9, 0.5, 0.7, 0.61])
    kp2 = torch.rand(2, 1, 2, 3, generator=torch.Generator().manual_seed(1))
    kp2[..., 2] = torch.tensor([0.45, 0.9])
    init85, targets, c, tracked, kmap, F, P = KF._seq_inputs(init, kp1, first, 0.6, [(1, 0)], (), dict(keypoints=kp2, kmap=second))
    assert (F, P, kmap.K) == (2, 1, 6) and kmap.sets == [(0, 4), (4, 6)] and tracked.tolist() == [[False], [True]]
    np.testing.assert_array_equal(targets, torch.cat([kp1, kp2], 2)[..., :2])
    want = np.array([0.9 ** 2 / 8, 0.0, 0.7 ** 2 / 8, 0.61 ** 2 / 8, 0.45 ** 2 / 4, 0.0])      # 0.5 < 0.6; 0.45 >= 0.4; weight 0
    np.testing.assert_allclose(c[0, 0].numpy(), want, rtol=1e-6)
    assert tuple(init85.shape) == (2, 1, 85)
