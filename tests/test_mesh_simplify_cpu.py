"""Mesh simplification without a device: the float64 reference (tests/mesh_simplify_reference.py) on shapes with known answers, the
cell representative of csrc/quadric_solve.hpp run ON THE HOST under AddressSanitizer and UBSan (tests/simplify_host.cpp) against
numpy.linalg.solve, the header's new prototypes, and the argument checks of multiply_amd/simplify.py that come before any launch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import mesh_simplify_reference as R
from tests import mesh_simplify_shapes as S
from tests import tolerances_simplify as T

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_shapes_are_what_the_tests_assume():
    v, f = S.tessellated_box()
    assert v.shape == (3458, 3) and f.shape == (6912, 3) and R.is_watertight(f)
    assert abs(R.volume(v, f) - 1.0) <= 1e-6                               # outward winding: the box's volume, positive
    v, f = S.two_sided_sheet()
    assert v.shape == (162, 3) and f.shape == (256, 3)


@pytest.mark.parametrize("shape, h, n_faces, n_duplicate", [("squashed", 0.11, 711, 1), ("squashed", 0.05, 2834, 8), ("sheet", 0.3, 18, 18)])
def test_reference_face_counts(shape, h, n_faces, n_duplicate):
    v, f = S.squashed(4) if shape == "squashed" else S.two_sided_sheet()
    r = R.simplify(v, f, h)
    info = r["info"]
    print(f"[reference {shape} h = {h}] {f.shape[0]} -> {r['faces'].shape[0]} faces, {info}")
    assert r["faces"].shape[0] == n_faces and info["n_duplicate"] == n_duplicate
    assert f.shape[0] - info["n_collapsed"] - info["n_duplicate"] == n_faces
    if shape == "sheet":
        assert f.shape[0] - info["n_collapsed"] == 36
    assert r["faces"].min() == 0 and r["faces"].max() == r["verts"].shape[0] - 1 and r["verts"].dtype == np.float32
    assert (np.diff(r["keys"][r["used"]]) > 0).all()                      # output vertices in ascending key order


def test_reference_squashed_sphere_stays_within_the_clamps_reach():
    """every output vertex lies in its cell, every input vertex of the cell too: an original vertex is within sqrt(3) h of its
    cell's representative, hence of the surface wherever the cell is referenced -- and here every cell is"""
    v, f = S.squashed(4)
    h = 0.11
    r = R.simplify(v, f, h)
    assert r["info"]["n_unreferenced"] == 0
    d = R.point_triangle_distance(v, r["verts64"][r["faces"]])
    print(f"[reference squashed(4) h = {h}] original vertices to the simplified surface: at most {d.max() / h:.4f} h (bound sqrt 3 h)")
    assert d.max() <= np.sqrt(3.0) * h


def test_reference_keeps_the_corners_of_a_box():
    v, f = S.tessellated_box()
    h = 0.13
    r = R.simplify(v, f, h)
    corners = S.box_corners()
    near = lambda pts: np.sqrt(((corners[:, None] - pts[None]) ** 2).sum(-1)).min(1) / h
    dq, dm = near(r["verts64"]), near(r["mean64"])
    ratio = R.volume(r["verts"], r["faces"]) / R.volume(v, f)
    print(f"[reference box h = {h}] {f.shape[0]} -> {r['faces'].shape[0]} faces; corners: quadric points within {dq.max():.2e} h, "
          f"cell means {dm.min():.2f} h .. {dm.max():.2f} h away; volume ratio {ratio:.6f}")
    assert R.is_watertight(r["faces"])
    assert dq.max() <= 0.01 and dm.min() >= 0.4
    assert abs(ratio - 1.0) <= 1e-3


def test_reference_cells_of_vertices_on_cell_faces_and_bad_input():
    v, f = S.lattice_sheet(0.125, 9)
    keys, cell = R.cell_ids(v, 0.125)
    assert keys.shape[0] == v.shape[0] and np.array_equal(R.unpack(keys[cell]), np.round((v - v[0]) / 0.125).astype(np.int64))
    bad = v.copy()
    bad[5, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        R.simplify(bad, f, 0.125)
    with pytest.raises(ValueError, match="fit"):
        R.simplify(v, f, 1e-7)
    with pytest.raises(ValueError, match="fit"):
        R.simplify(v, f, 0.125, lo=[0.0, 0.0, 0.0])                          # vertices below the origin


def test_reference_target_faces_bisection():
    v, f = S.squashed(4)
    r = R.simplify_to(v, f, 700)
    live = f.shape[0] - r["info"]["n_collapsed"]
    print(f"[reference target 700] walk {[(round(h, 5), n) for h, n in r['walk']]} -> {r['faces'].shape[0]} faces")
    assert r["info"]["passes"] == len(r["walk"]) <= 16 and abs(live - 700) <= 0.02 * 700 and r["walk"][-1][1] == live
    assert (r["info"]["n_cells"], live) == R.cluster_counts(v, f, r["info"]["cell"])


# ------------------------------------------------------------------------------------------------ the solve on the host, sanitized
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("simplify") / "simplify_host")
    cmd = [os.environ.get("HIPCC", "hipcc"), "-O1", "-g", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host",
           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(HERE, "simplify_host.cpp"),
           "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run_points(program, cases):
    """cases: [(A (6,), b (3,), mean (3,), lam, half)] -> solved (k,), x (k,3), x_free (k,3)"""
    text = "".join(" ".join("%.17g" % t for t in list(A) + list(b) + list(m) + [lam, half]) + "\n" for A, b, m, lam, half in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]            # a sanitizer report fails the run
    vals = np.array([[float(t) for t in line.split()] for line in r.stdout.strip().split("\n")])
    assert vals.shape == (len(cases), 7)
    return vals[:, 0].astype(int), vals[:, 1:4], vals[:, 4:7]


def packed(M):
    return [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]


def test_cell_representative_on_the_host_against_lapack(program):
    rng = np.random.RandomState(7)
    lam, h = 1e-3, 0.11
    half = 0.5 * h
    cases, kinds = [], []

    def add(kind, normals, point, mean, lam=lam):
        """faces with (unnormalised) normals through `point`: A = sum n n^T, b = A point"""
        A = normals.T @ normals
        cases.append((packed(A), A @ point, mean, lam, half))
        kinds.append((kind, A, A @ point, np.asarray(mean, float), lam))
    unit = lambda: (lambda d: d / np.linalg.norm(d))(rng.normal(0, 1, 3))
    inside = lambda: rng.uniform(-0.4, 0.4, 3) * h
    for k in range(60):                                                    # full rank, at three scales of the areas
        add("full rank", rng.normal(0, 1, (9, 3)) * 10.0 ** rng.uniform(-8, 2), inside(), inside())
    for k in range(60):                                                    # one dominant plane: the others 1e-3 .. 1e-9 of it
        add("plane", np.concatenate([np.outer(rng.uniform(0.5, 2, 6), unit()), rng.normal(0, 10.0 ** rng.uniform(-9, -3), (4, 3))]), inside(), inside())
    for k in range(60):                                                    # one dominant line: normals in a plane, plus dust
        e1, e2 = unit(), unit()
        add("line", np.concatenate([np.outer(rng.normal(0, 1, 6), e1) + np.outer(rng.normal(0, 1, 6), e2),
                                    rng.normal(0, 10.0 ** rng.uniform(-9, -3), (3, 3))]), inside(), inside())
    for k in range(20):                                                    # exact rank 1 and rank 2: only lam makes them solvable
        add("exact plane", np.outer(rng.uniform(0.5, 2, 5), unit()), inside(), inside())
        add("exact line", np.outer(rng.normal(0, 1, 6), unit()) + np.outer(rng.normal(0, 1, 6), unit()), inside(), inside())
    for k in range(10):                                                    # zero trace: the mean
        add("zero trace", np.zeros((4, 3)), inside(), inside())
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):   # the point outside the cell along 1, 2, 3 axes
        for sign in (-1.0, 1.0):
            p = inside()
            p[list(axes)] = sign * rng.uniform(0.8, 30.0, len(axes)) * h
            add("clamp %s" % (axes,), rng.normal(0, 1, (9, 3)), p, inside())
    solved, x, x_free = run_points(program, cases)
    worst = {}
    for (kind, A, b, mean, lam_), s, xc, xf in zip(kinds, solved, x, x_free):
        if kind == "zero trace":
            assert s == 0 and np.array_equal(xf, mean) and np.array_equal(xc, np.clip(mean, -half, half))
            continue
        l = lam_ * (A[0, 0] + A[1, 1] + A[2, 2]) / 3.0
        M = A + l * np.eye(3)
        assert np.linalg.cond(M) <= T.condition(lam_) * (1 + 1e-9), kind
        want = np.linalg.solve(M, b + l * mean)
        rel = np.linalg.norm(xf - want) / np.linalg.norm(want)
        worst[kind.split(" (")[0]] = max(worst.get(kind.split(" (")[0], 0.0), rel / T.solve_bound(lam_))
        assert s == 1 and rel <= T.solve_bound(lam_), (kind, rel, T.solve_bound(lam_))
        assert np.array_equal(xc, np.clip(xf, -half, half)), kind
        if kind.startswith("clamp"):
            axes = eval(kind[6:])
            assert all(abs(xc[a]) == half for a in axes) and (np.abs(xc) <= half).all(), (kind, xc / half)
    print(f"[quadric_point on the host vs LAPACK] {len(cases)} cells: |x - solve| / |solve| over the bound "
          f"{T.solve_bound(lam):.2e}: " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ header and host logic
def test_header_declares_the_entry_points_and_the_source_defines_them():
    from multiply_amd import hip
    protos = hip.header_prototypes()
    src = open(os.path.join(REPO, "multiply_amd", "csrc", "simplify.hip")).read()
    arity = dict(mp_simplify_keys=8, mp_simplify_count=6, mp_simplify_faces=9, mp_simplify_first=7, mp_simplify_quadrics=17,
                 mp_simplify_attr_mean=8)
    for name, n in arity.items():
        assert name in protos and len(protos[name][1]) == n and protos[name][1][-1] is hip.DevPtr, name
        assert re.search(r'extern "C" int %s\(' % name, src), name
    hdr = open(hip.HEADER_PATH).read()
    assert int(re.search(r"#define MP_SIMPLIFY_BITS (\d+)", hdr).group(1)) == hip.SIMPLIFY_BITS == R.BITS
    assert int(re.search(r"#define MP_SIMPLIFY_LANES (\d+)", hdr).group(1)) == hip.SIMPLIFY_LANES
    assert "fp contract(off)" in src                                        # n = 0 exactly for equal edge vectors: no FMA


def test_arguments_are_checked_before_a_device_is_needed():
    from multiply_amd import simplify
    v, f = S.squashed(1)
    with pytest.raises(ValueError, match="exactly one"):
        simplify.simplify_mesh(v, f)
    with pytest.raises(ValueError, match="exactly one"):
        simplify.simplify_mesh(v, f, cell=0.1, target_faces=10)
    with pytest.raises(ValueError, match="lam"):
        simplify.simplify_mesh(v, f, cell=0.1, lam=0.0)
    box = (v.min(0), v.max(0))
    assert simplify.bisection_ends(box) == R.bisection_ends(v)
    flat = (np.zeros(3, np.float32), np.array([1.0, 0.0, 3.0], np.float32))
    assert simplify.bisection_ends(flat) == (3.0 / 2 ** 20, 3.0)
    with pytest.raises(ValueError, match="fit"):
        simplify._cell_args(1e-8, box[0], box)
    with pytest.raises(ValueError, match="positive"):
        simplify._cell_args(-1.0, box[0], box)
    assert simplify._cell_args(0.11, box[0], box)[:2] == (float(np.float32(0.11)), float(np.float32(1.0) / np.float32(0.11)))


def test_tool_matches_folders_by_name(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import simplify_mesh as tool
    finally:
        sys.path.pop(0)
    a = tmp_path / "in"
    a.mkdir()
    for n in ("0001_canonical.ply", "0000_deformed.PLY", "notes.txt"):
        (a / n).write_bytes(b"")
    (a / "dir.ply").mkdir()
    jobs = tool.jobs_of(str(a), str(tmp_path / "out"))
    assert jobs == [(str(a / "0000_deformed.PLY"), str(tmp_path / "out" / "0000_deformed.PLY")),
                    (str(a / "0001_canonical.ply"), str(tmp_path / "out" / "0001_canonical.ply"))]
    assert tool.jobs_of(str(a / "0001_canonical.ply"), str(tmp_path / "x.ply")) == [(str(a / "0001_canonical.ply"), str(tmp_path / "x.ply"))]
    args = tool.parser().parse_args(["in.ply", "out.ply", "--faces", "5000"])
    assert args.faces == 5000 and args.cell is None
    with pytest.raises(SystemExit):
        tool.parser().parse_args(["in.ply", "out.ply", "--faces", "5000", "--cell", "0.1"])
    with pytest.raises(SystemExit):
        tool.parser().parse_args(["in.ply", "out.ply"])
