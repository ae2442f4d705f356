"""Registration without a device: the float64 reference (tests/registration_reference.py) pinned on problems with known answers,
the Gauss-Newton step of csrc/reg_solve.hpp run ON THE HOST under AddressSanitizer and UBSan (tests/registration_host.cpp) against
numpy.linalg.solve, and the host logic of multiply_amd/registration.py, metrics.mesh_metrics(align=...) and tools/eval_meshes.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from multiply_amd import registration as reg
from tests import registration_reference as RR
from tests import registration_shapes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("similarity", [False, True])
def test_reference_umeyama_recovers_exact_pairs(similarity):
    rng = np.random.RandomState(1)
    for _ in range(20):
        p = rng.normal(0, 1, (40, 3)) * rng.uniform(0.1, 3) + rng.normal(0, 2, 3)
        R0, t0 = RS.rotation(rng.normal(0, 1, 3), rng.uniform(0, 179)), rng.normal(0, 1, 3)
        s0 = rng.uniform(0.3, 3.0) if similarity else 1.0
        q = s0 * p @ R0.T + t0
        w = rng.uniform(0.0, 2.0, 40) * (rng.uniform(0, 1, 40) > 0.2)
        s, Rm, t, _, _ = RR.umeyama(p, q, w, similarity)
        assert abs(s - s0) <= 1e-12 and np.abs(Rm - R0).max() <= 1e-12 and np.abs(t - t0).max() <= 1e-12 * max(1.0, np.abs(t0).max())


def test_reference_umeyama_gives_a_proper_rotation_on_degenerate_pairs():
    rng = np.random.RandomState(2)
    p = rng.normal(0, 1, (30, 3))
    flat = p * np.array([1.0, 1.0, 0.0])
    line = np.outer(rng.normal(0, 1, 30), [0.3, -0.5, 0.8])
    R0 = RS.rotation([1, 2, -1], 40)
    for name, a, b in (("mirrored", p, p * np.array([-1.0, 1.0, 1.0])), ("coplanar", flat, flat @ R0.T), ("collinear", line, line @ R0.T)):
        s, Rm, t, _, _ = RR.umeyama(a, b, None, True)
        assert np.isfinite(Rm).all() and abs(np.linalg.det(Rm) - 1.0) <= 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12, name
        if name != "mirrored":               # the pairs are an exact rigid motion of each other: it is attained
            assert np.abs(s * a @ Rm.T + t - b).max() <= 1e-12, name


def area_samples(v, f, n, seed):
    """n area-uniform points on the mesh, float64 (numpy): face by the area CDF, barycentrics by the square-root map"""
    rng = np.random.RandomState(seed)
    fv = np.asarray(v, np.float64)[f]
    area = 0.5 * np.linalg.norm(np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]), axis=1)
    k = np.minimum(np.searchsorted(np.cumsum(area) / area.sum(), rng.uniform(0, 1, n)), len(f) - 1)
    r1, r2 = np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 1, n)
    return (1 - r1)[:, None] * fv[k, 0] + (r1 * (1 - r2))[:, None] * fv[k, 1] + (r1 * r2)[:, None] * fv[k, 2]


def test_reference_icp_recovers_an_exact_copy_within_six_iterations():
    """bumpy-1280 against its copy under 8 degrees about (1, 2, -1), t = (0.03, -0.02, 0.025), s = 1.07, 800 samples per side, from
    the identity: point-to-plane reaches max vertex error <= 1e-7 within 6 iterations"""
    v, f = RS.bumpy(3)
    R0, t0, s0 = RS.rotation([1, 2, -1], 8.0), np.array([0.03, -0.02, 0.025]), 1.07
    w = RS.moved(v, R0, t0, s0)
    ps, qs = area_samples(v, f, 800, 0), area_samples(w, f, 800, 1)
    hist = []
    RR.icp((v, f), (w, f), ps, qs, True, max_iters=6, tol=0.0, init=(1.0, np.eye(3), np.zeros(3)), history=hist)
    want = s0 * v.astype(np.float64) @ R0.T + t0
    errs = [np.abs(RR.apply(st, v) - want).max() for st in hist]
    print("[reference ICP, exact copy] max vertex error per iteration:", " ".join(f"{e:.2e}" for e in errs))
    assert len(errs) == 6 and min(errs) <= 1e-7 and errs[-1] <= 1e-7


# ------------------------------------------------------------------------------------------------ the step on the host, sanitized
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("registration") / "registration_host")
    cmd = [os.environ.get("HIPCC", "hipcc"), "-O1", "-g", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(HERE, "registration_host.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run_steps(program, cases):
    """cases: [(similarity, reject, tol, sums (40,), state (32,))] -> flags, deltas (k,7), states (k,32)"""
    num = lambda a: " ".join("%.17g" % v for v in a)
    text = "".join(f"{int(s)} {rej:.17g} {tol:.17g} {num(sums)} {num(st)}\n" for s, rej, tol, sums, st in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]          # a sanitizer report fails the run
    vals = np.array([[float(t) for t in line.split()] for line in r.stdout.strip().split("\n")])
    assert vals.shape == (len(cases), 1 + 7 + RR.STATE)
    return vals[:, 0].astype(int), vals[:, 1:8], vals[:, 8:]


sums_from = RR.sums_from


def test_step_routine_on_the_host_against_lapack(program):
    rng = np.random.RandomState(3)
    st0 = RR.new_state(1.1, RS.rotation([0.2, 1, -0.4], 12), [0.1, -0.2, 0.3], [-1, -1.5, -0.5], [1.2, 1.4, 0.9])
    cases, kinds = [], []

    def add(kind, A, b, similarity, n_acc=100.0):
        cases.append((similarity, 3.0, 1e-6, sums_from(A, b, n_acc), st0))
        kinds.append((kind, A, b, similarity))
    for k in range(60):                                       # random SPD, 6 x 6 and 7 x 7
        B = rng.normal(0, 1, (12, 7))
        add("spd", B.T @ B, rng.normal(0, 1e-2, 7), k % 2)
    for k in range(40):                                       # ill-scaled: D A D with D over 12 orders
        B = rng.normal(0, 1, (12, 7))
        D = np.diag(10.0 ** rng.uniform(-6, 6, 7))
        add("ill-scaled", D @ (B.T @ B) @ D, D @ rng.normal(0, 1e-2, 7) * 1e-6, k % 2)
    for k in range(20):                                       # singular: rank 4, and an exactly zero row and column
        B = rng.normal(0, 1, (4, 7))
        add("singular", B.T @ B, rng.normal(0, 1e-2, 7), k % 2)
        A = rng.normal(0, 1, (12, 7))
        A[:, 2] = 0.0
        add("singular", A.T @ A, rng.normal(0, 1e-2, 7), k % 2)
    for k in range(6):                                        # fewer than 7 rows: a good matrix, too few accepted pairs
        B = rng.normal(0, 1, (12, 7))
        add("few", B.T @ B, rng.normal(0, 1e-2, 7), k % 2, n_acc=float(k))
    flags, deltas, states = run_steps(program, cases)
    worst = {"spd": 0.0, "ill-scaled": 0.0}
    for (kind, A, b, similarity), flag, d, st in zip(kinds, flags, deltas, states):
        m = 7 if similarity else 6
        if kind in ("singular", "few"):
            assert flag == RR.DEGENERATE and np.array_equal(st[:13], st0[:13]) and (d == 0).all(), kind
            continue
        want = np.linalg.solve(A[:m, :m], b[:m])
        rel = np.linalg.norm(d[:m] - want) / np.linalg.norm(want)
        bound = np.linalg.cond(A[:m, :m]) * EPS
        worst[kind] = max(worst[kind], rel / bound)
        assert flag in (0, RR.CONVERGED) and rel <= bound, (kind, rel, bound)
        if kind == "spd":                                      # the composed state as the reference composes it (cond ~ 10^2)
            ref, _ = RR.step(sums_from(A, b), st0, similarity)
            assert np.abs(st - ref).max() <= 1e-12, np.abs(st - ref).max()
    print(f"[reg_step on the host vs LAPACK] {len(cases)} systems: |delta - solve| / (cond 2^-52 |solve|) at most "
          f"{worst['spd']:.3f} (SPD), {worst['ill-scaled']:.3f} (ill-scaled)")


def test_step_routine_leaves_a_flagged_state_alone(program):
    rng = np.random.RandomState(4)
    B = rng.normal(0, 1, (12, 7))
    for flag in (RR.CONVERGED, RR.DEGENERATE):
        st = RR.new_state(0.9, RS.rotation([1, 0, 1], 5), [0.0, 0.1, 0.2], [-1, -1, -1], [1, 1, 1])
        st[RR.FLAG], st[RR.RMS], st[RR.ITERS] = flag, 0.123, 4
        flags, _, states = run_steps(program, [(1, 3.0, 1e-6, sums_from(B.T @ B, rng.normal(0, 1, 7)), st)])
        assert flags[0] == flag and np.array_equal(states[0], st)


# ------------------------------------------------------------------------------------------------ host logic, no device
def test_similarity_algebra():
    """coordinates, translations and scales of size <= 1, so that a handful of double roundings stay below 1e-15"""
    rng = np.random.RandomState(5)
    T = [reg.Similarity(rng.uniform(0.8, 1.25), RS.rotation(rng.normal(0, 1, 3), rng.uniform(0, 170)), rng.uniform(-0.3, 0.3, 3)) for _ in range(3)]
    p = rng.uniform(-0.5, 0.5, (50, 3))
    for A in T:
        assert np.abs(A.inverse().apply(A.apply(p)) - p).max() <= 1e-15
        assert np.abs(A.compose(A.inverse()).matrix - np.eye(4)).max() <= 1e-15
        assert np.allclose(A.matrix @ np.append(p[0], 1.0), np.append(A.apply(p[0]), 1.0), rtol=0, atol=1e-15)
        B = reg.Similarity.from_matrix(A.matrix)
        assert abs(B.scale - A.scale) <= 1e-15 and np.abs(B.R - A.R).max() <= 1e-15 and np.array_equal(B.t, A.t)
    left, right = T[0].compose(T[1]).compose(T[2]), T[0].compose(T[1].compose(T[2]))
    assert np.abs(left.matrix - right.matrix).max() <= 1e-15
    assert np.abs(T[0].compose(T[1]).apply(p) - T[0].apply(T[1].apply(p))).max() <= 1e-15
    import torch
    assert torch.equal(T[0].apply(torch.from_numpy(p)), torch.from_numpy(T[0].apply(p)))
    assert T[0].apply(torch.from_numpy(p).float()).dtype == torch.float32


def test_register_and_metrics_reject_bad_arguments_before_touching_a_device():
    from multiply_amd import metrics
    v, f = RS.bumpy(2)
    with pytest.raises(ValueError, match="align"):
        metrics.mesh_metrics((v, f), (v, f), n_samples=10, align="affine")
    with pytest.raises(ValueError, match="align"):
        metrics.mesh_metrics((v, f), (v, f), n_samples=10, align=np.eye(4))
    with pytest.raises(ValueError, match="kind"):
        reg.register((v, f), (v, f), kind="affine")
    with pytest.raises(ValueError, match="directions"):
        reg.register((v, f), (v, f), directions="sideways")
    with pytest.raises(ValueError, match="init"):
        reg.register((v, f), (v, f), init="pca")
    with pytest.raises(ValueError, match="as many"):
        reg.register_sequence([(v, f)], [])


def test_eval_meshes_matches_folders_by_name_and_takes_means(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import eval_meshes as E
    finally:
        sys.path.pop(0)
    a, b = tmp_path / "pred", tmp_path / "gt"
    a.mkdir(), b.mkdir()
    for d, names in ((a, ["0002.ply", "0000.ply", "0001.PLY", "only_pred.ply", "notes.txt"]), (b, ["0000.ply", "0002.ply", "0001.PLY", "only_gt.ply"])):
        for n in names:
            (d / n).write_bytes(b"")
    (a / "dir.ply").mkdir()
    pairs, unmatched = E.match_folders(str(a), str(b))
    assert [p[0] for p in pairs] == ["0000.ply", "0001.PLY", "0002.ply"]
    assert all(p[1] == str(a / p[0]) and p[2] == str(b / p[0]) for p in pairs)
    assert unmatched == {"pred": ["only_pred.ply"], "gt": ["only_gt.ply"]}
    m = E.mean_of([dict(chamfer=1.0, f_score=[0.5, 1.0], n_samples=10, align=dict(kind="rigid")),
                   dict(chamfer=3.0, f_score=[0.0, 0.5], n_samples=10, align=dict(kind="rigid"))])
    assert m == dict(chamfer=2.0, f_score=[0.25, 0.75], n_samples=10.0)
    v, f = RS.bumpy(2)
    E.write_ply(str(tmp_path / "m.ply"), v, f)
    from multiply_amd.metrics import load_ply
    v2, f2 = load_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(v2, v) and np.array_equal(f2, f)
