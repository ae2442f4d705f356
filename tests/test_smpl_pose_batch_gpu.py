"""SMPLServer.pose_batch (mp_smpl_pose_batch): N parameter rows in two launches against the CPU oracle row by row, the
independence of a row from its batch, determinism, skipped outputs, and the single-row path."""
import numpy as np
import pytest
import torch

from multiply_amd import hip
from oracle import multiply_oracle as O
from tests import tolerances_pose_metrics as TOL
from tests.util import t32

pytestmark = pytest.mark.gpu

R = hip.SMPL_BATCH_ROWS                 # rows per pass of the vertex kernel
N_ALL = 2 * R + 1


@pytest.fixture(scope="module")
def setup(smpl_tables):
    from multiply_amd.smpl import SMPLServer
    from multiply_amd.synthetic import make_scene
    sp = make_scene(2, seed=0, H=16, W=16)["smpl_params"][0]
    betas = [sp[0, 76:], sp[1, 76:]]                                # two different shapes in one batch
    sv = SMPLServer(gender="male", betas=betas[0], smpl_tables=smpl_tables)
    rng = np.random.RandomState(5)
    rows = np.zeros((N_ALL, 86), np.float32)
    for i in range(N_ALL):
        std = (0.0, 0.3, 0.6)[i % 3]                                # row 0: zero thetas
        rows[i, 0] = (1.0, 1.2)[(i // 3) % 2]
        rows[i, 1:4] = rng.normal(0, 0.3, 3)
        rows[i, 4:76] = rng.normal(0, 1, 72) * std
        rows[i, 76:] = betas[(i // 2) % 2]
    return sv, O.SMPLServerOracle(smpl_tables, betas[0]), rows, {}


def oracle_row(setup, i, absolute):
    sv, ref, rows, cache = setup
    if (i, absolute) not in cache:
        r = t32(rows[i])
        cache[(i, absolute)] = O.smpl_server_forward(ref.T, r[0], r[1:4], r[4:76], r[76:], None if absolute else ref.tfs_c_inv)
    return cache[(i, absolute)]


def err(got, want):
    return (got.double().cpu() - want.double()).abs().max().item()


def test_rows_cover_the_cases(setup):
    rows = setup[2]
    assert not rows[0, 4:76].any() and rows[0, 0] == 1.0
    # zero thetas, N(0, 0.3) and N(0, 0.6) x two scales x two shapes: all twelve combinations
    assert len({(i % 3, float(rows[i, 0]), tuple(rows[i, 76:78])) for i in range(N_ALL)}) == 12
    assert 0.2 < rows[1, 4:76].std() < 0.4 and 0.45 < rows[2, 4:76].std() < 0.75


@pytest.mark.parametrize("absolute", [False, True])
@pytest.mark.parametrize("N", [1, 3, R + 1, 2 * R + 1])
def test_against_the_oracle(setup, N, absolute):
    sv, ref, rows, _ = setup
    out = sv.pose_batch(torch.from_numpy(rows[:N]).cuda(), absolute=absolute)
    assert out["verts"].shape == (N, 6890, 3) and out["joints"].shape == (N, 24, 3) and out["tfs"].shape == (N, 24, 4, 4)
    worst = [0.0, 0.0, 0.0]
    for i in range(N):
        want = oracle_row(setup, i, absolute)
        e = (err(out["verts"][i], want["smpl_verts"]), err(out["joints"][i], want["smpl_jnts"]), err(out["tfs"][i], want["smpl_tfs"]))
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"[pose_batch vs oracle] N {N} absolute {absolute}: verts {worst[0]:.2e} joints {worst[1]:.2e} tfs {worst[2]:.2e}")
    assert worst[0] < TOL.POSE_POINTS and worst[1] < TOL.POSE_POINTS and worst[2] < TOL.POSE_TFS


def test_a_row_has_the_same_bits_alone_and_inside_a_batch(setup):
    sv, _, rows, _ = setup
    probe = torch.from_numpy(rows[5:6]).cuda()                      # N(0, 0.6), scale 1.2
    alone = sv.pose_batch(probe)
    for pos in (0, R, N_ALL - 1, 7):                                # first, a middle one on a pass boundary, last, inside a pass
        batch = torch.from_numpy(np.roll(rows, 3, axis=0)).cuda()
        batch[pos] = probe[0]
        out = sv.pose_batch(batch)
        for k in ("verts", "joints", "tfs"):
            assert torch.equal(out[k][pos], alone[k][0]), (pos, k)


def test_two_calls_and_split_calls_give_identical_bits(setup):
    sv, _, rows, _ = setup
    p = torch.from_numpy(rows).cuda()
    a, b, c = sv.pose_batch(p), sv.pose_batch(p), sv.pose_batch(p, rows_per_call=5)
    for k in ("verts", "joints", "tfs"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_each_output_can_be_skipped(setup):
    sv, _, rows, _ = setup
    p = torch.from_numpy(rows[:R + 1]).cuda()
    full = sv.pose_batch(p)
    for want in (("verts",), ("joints",), ("tfs",), ("joints", "tfs"), ("verts", "tfs")):
        out = sv.pose_batch(p, want=want)
        assert sorted(out) == sorted(want)
        for k in want:
            assert torch.equal(out[k], full[k]), (want, k)
    with pytest.raises(ValueError, match="want"):
        sv.pose_batch(p, want=("faces",))
    with pytest.raises(ValueError, match="params"):
        sv.pose_batch(p[:, :85])
    assert sv.pose_batch(p[:0])["verts"].shape == (0, 6890, 3)


def test_against_the_single_row_path(setup):
    sv, _, rows, _ = setup
    N = R + 1
    p = torch.from_numpy(rows[:N]).cuda()
    for absolute in (False, True):
        out = sv.pose_batch(p, absolute=absolute)
        f32 = dict(dtype=torch.float32, device="cuda")
        worst = [0.0, 0.0, 0.0]
        for i in range(N):
            v, t, j = torch.empty(6890, 3, **f32), torch.empty(24, 4, 4, **f32), torch.empty(24, 3, **f32)
            sv.pose_into(p[i], v, t, j, absolute=absolute)
            e = (err(out["verts"][i], v.cpu()), err(out["joints"][i], j.cpu()), err(out["tfs"][i], t.cpu()))
            worst = [max(a, b) for a, b in zip(worst, e)]
        print(f"[pose_batch vs pose_into] absolute {absolute}: verts {worst[0]:.2e} joints {worst[1]:.2e} tfs {worst[2]:.2e}")
        assert worst[0] < 2 * TOL.POSE_POINTS and worst[1] < 2 * TOL.POSE_POINTS and worst[2] < 2 * TOL.POSE_TFS


def test_forward_only(setup):
    sv, _, rows, _ = setup
    p = torch.from_numpy(rows[:2]).cuda().requires_grad_(True)
    out = sv.pose_batch(p)
    assert not any(t.requires_grad for t in out.values())
