"""The 3 x 3 Procrustes routine of csrc/pose_metrics.hip (one-sided Jacobi SVD, the rotation without a third singular vector) run
ON THE HOST: tests/procrustes_host.cpp is compiled around it with AddressSanitizer and UBSan and compared with numpy.linalg.svd --
Umeyama's R = V D U^T and tr(S D) -- on well-conditioned, mirrored, rank-2, rank-1, zero and badly scaled matrices."""
import os
import subprocess

import numpy as np
import pytest

from multiply_amd import pose_metrics  # noqa: F401  (the module this routine serves)

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("procrustes") / "procrustes_host")
    cmd = [os.environ.get("HIPCC", "hipcc"), "-O1", "-g", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(HERE, "procrustes_host.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(program, Hs):
    text = "\n".join(" ".join("%.17g" % v for v in H.reshape(-1)) for H in Hs) + "\n"
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]          # a sanitizer report fails the run
    vals = np.array([[float(t) for t in line.split()] for line in r.stdout.strip().split("\n")])
    assert vals.shape == (len(Hs), 10)
    return vals[:, 0], vals[:, 1:].reshape(-1, 3, 3)


def umeyama(H):
    U, S, Vt = np.linalg.svd(H)
    V, D = Vt.T, np.ones(3)
    if np.linalg.det(V @ U.T) < 0:
        D[2] = -1.0
    return (S * D).sum(), V @ np.diag(D) @ U.T, S


def test_procrustes_routine_against_lapack(program):
    rng = np.random.RandomState(0)
    Hs = [rng.normal(0, 1, (3, 3)) * 10.0 ** rng.uniform(-6, 6) for _ in range(300)]                    # either sign of det H
    spd = [a @ a.T for a in rng.normal(0, 1, (50, 3, 3))]
    Hs += [c @ np.diag([-1.0, 1.0, 1.0]) for c in spd]                                                  # mirrored clouds
    Hs += [np.outer(rng.normal(0, 1, 3), rng.normal(0, 1, 3)) + np.outer(rng.normal(0, 1, 3), rng.normal(0, 1, 3)) for _ in range(50)]
    Hs += [c * np.array([[1.0], [1.0], [0.0]]) for c in spd]                                            # a coplanar cloud: a zero row
    n_unique = len(Hs)
    Hs += [np.outer(rng.normal(0, 1, 3), rng.normal(0, 1, 3)) for _ in range(20)]                       # collinear: R is not unique
    Hs += [np.zeros((3, 3)), np.eye(3), -np.eye(3), np.diag([2.0, 2.0, 2.0]), np.diag([1.0, 1.0, 1e-300])]
    tr, R = run(program, Hs)
    worst = [0.0, 0.0, 0.0, 0.0]
    for k, H in enumerate(Hs):
        want_tr, want_R, S = umeyama(H)
        scale = max(S[0], 1e-300)
        e_tr = abs(tr[k] - want_tr) / scale
        e_obj = abs(np.trace(R[k] @ H) - want_tr) / scale           # R attains the maximum of tr(R H) over the rotations
        e_rot = np.abs(R[k] @ R[k].T - np.eye(3)).max() + abs(np.linalg.det(R[k]) - 1.0)
        worst = [max(a, b) for a, b in zip(worst, (e_tr, e_obj, e_rot, 0.0))]
        assert np.isfinite(R[k]).all() and e_tr <= 1e-14 and e_obj <= 1e-14 and e_rot <= 1e-14, (k, e_tr, e_obj, e_rot)
        gap = (S[1] + (S[2] if np.linalg.det(H) >= 0 else -S[2])) / scale   # R is unique, and well conditioned, when this is not small
        if k < n_unique and gap > 1e-3:
            e_R = np.abs(R[k] - want_R).max()
            worst[3] = max(worst[3], e_R)
            assert e_R <= 1e-12 / gap, (k, e_R, gap)
    print(f"[procrustes on the host vs LAPACK] {len(Hs)} matrices: tr(S D) {worst[0]:.2e}  tr(R H) {worst[1]:.2e}  "
          f"orthogonality {worst[2]:.2e}  R {worst[3]:.2e}")
