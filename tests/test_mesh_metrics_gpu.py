"""Mesh-to-mesh metrics on the device (multiply_amd/metrics.py, mp_mesh_metric_reduce) against the float64 reference
(tests/mesh_metrics_reference.py), which is fed the device's own sample points and reported faces: the query and the reduction
are under test, not the sampler (tests/test_smpl_init_gpu.py has that)."""
import numpy as np
import pytest
import torch

from tests import mesh_metrics_reference as R
from tests import mesh_metrics_shapes as S
from tests import tolerances_mesh_metrics as TOL

pytestmark = pytest.mark.gpu

N = 4096
SHIFT = np.array([0.02, -0.015, 0.01], np.float32)
THRESHOLDS = (0.5, 1.2, 2.0)                # in the scaled unit (unit_scale 100): the shift is 2.7 long


def _pair():
    v, f = S.squashed(2)
    return (v, f), ((v + SHIFT).astype(np.float32), f)


def _shortest_edge(v, f):
    fv = np.asarray(v, np.float64)[np.asarray(f)]
    return min(np.linalg.norm(fv[:, i] - fv[:, (i + 1) % 3], axis=1).min() for i in range(3))


@pytest.fixture(scope="module")
def run():
    """mesh_metrics of squashed(2) against a translated copy, its details, and the reference on the same samples"""
    from multiply_amd import metrics
    pred, gt = _pair()
    details = {}
    got = metrics.mesh_metrics(pred, gt, n_samples=N, thresholds=THRESHOLDS, seed=3, unit_scale=100.0, iou_resolution=12, details=details)
    a, c = details["accuracy"], details["completeness"]
    cpu = lambda t: t.cpu().numpy()
    want = R.metrics(pred, gt, (cpu(a["points"]), cpu(a["sample_face"])), (cpu(c["points"]), cpu(c["sample_face"])), THRESHOLDS, 100.0, 12,
                     reported=(cpu(a["face"]), cpu(c["face"])))
    return dict(pred=pred, gt=gt, got=got, want=want, details=details)


def test_metric_reduce_matches_float64_on_the_devices_own_query(run):
    from multiply_amd import hip
    d = run["details"]["accuracy"]
    gv, gf = run["gt"]
    fn = hip.fit_area_cdf(torch.from_numpy(gv[gf]).cuda())[1]
    # a few samples without an answer: left out and counted
    d2 = torch.cat([d["d2"], torch.full((5,), float("inf"), device="cuda")])
    face = torch.cat([d["face"], torch.full((5,), -1, dtype=torch.int32, device="cuda")])
    nrm = torch.cat([d["normals"], torch.zeros(5, 3, device="cuda")])
    tau = [0.01, 0.02, 0.03, 1e-9, 10.0]
    got = hip.mesh_metric_reduce(d2, face, nrm, fn, tau).cpu().numpy()
    again = hip.mesh_metric_reduce(d2, face, nrm, fn, tau).cpu().numpy()
    assert np.array_equal(got, again)
    tau32 = np.array(tau, np.float32).astype(np.float64)
    want = R.reduce(d2.cpu().numpy(), face.cpu().numpy(), nrm.cpu().numpy(), fn.cpu().numpy(), tau32)
    M = TOL.coordinate_scale(d["points"].cpu().numpy(), gv)
    for k, name in enumerate(("mean distance", "mean squared distance", "max", "mean n.n'", "mean |n.n'|")):
        print(f"[reduce] {name}: {got[k]:.9e} vs float64 {want[k]:.9e}, off {abs(got[k] - want[k]):.2e} (bound {TOL.mean(M, want[k]):.2e})")
    for k in (0, 1, 3, 4):
        assert abs(got[k] - want[k]) <= TOL.mean(M, want[k])
    assert got[2] == float(np.sqrt(d2.cpu().numpy()[:-5]).max())            # exact: the largest fp32 square root
    assert got[5] == N and got[6] == 5 and want[5] == N
    d64 = np.sqrt(d2.cpu().numpy()[:-5].astype(np.float64))
    for k, t in enumerate(tau32):
        close = int((np.abs(d64 - t) <= TOL.delta(M)).sum())
        print(f"[reduce] threshold {t:g}: {got[7 + k]:.0f} vs {want[7 + k]:.0f}; {close} samples within delta of it")
        assert abs(got[7 + k] - want[7 + k]) <= close
    assert got[10] == 0 and got[11] == N
    empty = hip.mesh_metric_reduce(d2[:0], face[:0], nrm[:0], fn, tau[:2]).cpu().numpy()
    assert empty.shape == (9,) and not empty.any()
    none = hip.mesh_metric_reduce(d2[-5:], face[-5:], nrm[-5:], fn, ()).cpu().numpy()
    assert none.tolist() == [0, 0, 0, 0, 0, 0, 5]


def test_mesh_metrics_match_the_reference_entry_by_entry(run):
    got, want, s = run["got"], run["want"], 100.0
    (pv, _), (gv, _) = run["pred"], run["gt"]
    M = TOL.coordinate_scale(pv, gv)
    delta = TOL.delta(M)
    assert set(want) <= set(got) and got["n_left_out"] == 0 and got["n_samples"] == N
    dmax = want["hausdorff"] / s
    bound = {k: s * TOL.mean(M, want[k] / s) for k in ("accuracy", "completeness", "p2s", "chamfer", "hausdorff")}
    # a squared distance: (d + e)^2 - d^2 <= 2 d e + e^2 per sample, two means summed
    bound["chamfer_sq"] = s * s * 2 * (2 * dmax * delta + delta * delta + 4 * TOL.FLT_EPSILON * dmax * dmax)
    # normals: the reference takes the device's reported faces, so only the fp32 normals and their dot product differ
    bound["normal_consistency"] = bound["normal_consistency_signed"] = 2 * TOL.normal(M, _shortest_edge(*run["pred"]))
    for k, b in bound.items():
        print(f"[metrics] {k}: {got[k]:.9e} vs float64 {want[k]:.9e}, off {abs(got[k] - want[k]):.2e} (bound {b:.2e})")
        assert abs(got[k] - want[k]) <= b, k
    assert got["p2s"] == got["completeness"] and got["thresholds"] == list(THRESHOLDS)
    # a threshold count may differ by the samples whose float64 distance is within delta of it
    close = {}
    for name, key in (("accuracy", "precision"), ("completeness", "recall")):
        d = run["details"][name]
        other = run["gt"] if name == "accuracy" else run["pred"]
        d64 = np.sqrt(R.closest(d["points"].cpu().numpy(), other[0][other[1]])[0])
        close[key] = [int((np.abs(d64 - t / s) <= delta).sum()) / N for t in THRESHOLDS]
        for k, t in enumerate(THRESHOLDS):
            print(f"[metrics] {key}({t}): {got[key][k]:.6f} vs {want[key][k]:.6f}; within delta of the threshold: {close[key][k] * N:.0f} samples")
            assert abs(got[key][k] - want[key][k]) <= close[key][k] + 1e-12
    assert 0 < want["precision"][0] < want["precision"][2] <= 1.0                 # the thresholds cut through the distribution
    for k in range(len(THRESHOLDS)):                                               # |dF| <= 2 (|dP| + |dR|)
        assert abs(got["f_score"][k] - want["f_score"][k]) <= 2 * (close["precision"][k] + close["recall"][k]) + 1e-12
    print(f"[metrics] volume_iou {got['volume_iou']:.6f} vs float64 {want['volume_iou']:.6f}")
    lat = R.lattice(np.minimum(pv.min(0), gv.min(0)), np.maximum(pv.max(0), gv.max(0)), 12)
    near = sum(int((np.sqrt(R.closest(lat, v[f])[0]) <= delta).sum()) for v, f in (run["pred"], run["gt"]))
    assert abs(got["volume_iou"] - want["volume_iou"]) <= (0.0 if near == 0 else 2 * near / 12 ** 3 / want["volume_iou"])
    assert 0.5 < got["volume_iou"] < 1.0


def test_mesh_metrics_are_symmetric_and_repeatable(run):
    from multiply_amd import metrics
    kw = dict(n_samples=N, thresholds=THRESHOLDS, seed=3, unit_scale=100.0, iou_resolution=12)
    got = run["got"]
    assert metrics.mesh_metrics(run["pred"], run["gt"], **kw) == got          # the same seed: the same bits
    swapped = metrics.mesh_metrics(run["gt"], run["pred"], **kw)
    assert swapped["accuracy"] == got["completeness"] and swapped["completeness"] == got["accuracy"]
    assert swapped["precision"] == got["recall"] and swapped["recall"] == got["precision"] and swapped["f_score"] == got["f_score"]
    for k in ("chamfer", "chamfer_sq", "hausdorff", "normal_consistency", "normal_consistency_signed", "volume_iou"):
        assert swapped[k] == got[k], k
    assert metrics.mesh_metrics(run["pred"], run["gt"], **{**kw, "seed": 4})["accuracy"] != got["accuracy"]


def test_brute_force_and_index_give_equal_dicts(run):
    from multiply_amd import metrics
    kw = dict(n_samples=N, thresholds=THRESHOLDS, seed=3, unit_scale=100.0, iou_resolution=12)
    assert metrics.mesh_metrics(run["pred"], run["gt"], index_mode="brute", **kw) == run["got"]
    assert metrics.mesh_metrics(run["pred"], run["gt"], index_mode="index", **kw) == run["got"]
    pts = run["details"]["accuracy"]["points"]
    b, i = metrics.directed(pts, run["gt"], "brute"), metrics.directed(pts, run["gt"], "index")
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(b, i))


def test_surface_samples_lie_on_their_faces_and_follow_the_generator():
    from multiply_amd import metrics
    v, f = S.squashed(2)
    gen = lambda: torch.Generator(device="cuda").manual_seed(7)
    pts, nrm, fid = metrics.surface_samples((v, f), 1000, gen())
    again = metrics.surface_samples((torch.from_numpy(v), torch.from_numpy(f)), 1000, gen())
    assert all(torch.equal(x, y) for x, y in zip((pts, nrm, fid), again))
    assert pts.shape == (1000, 3) and nrm.shape == (1000, 3) and fid.shape == (1000,) and fid.dtype == torch.int32
    off = np.sqrt(R.closest_points_paired(pts.cpu().numpy(), v[f][fid.cpu().numpy()])[0])
    assert off.max() <= TOL.delta(TOL.coordinate_scale(v))
    assert np.abs(nrm.cpu().numpy() - R.face_normals(v[f])[fid.cpu().numpy()]).max() <= TOL.normal(TOL.coordinate_scale(v), _shortest_edge(v, f))
    assert metrics.surface_samples((v, f), 0, gen())[0].shape == (0, 3)


def test_extracted_sphere_against_an_icosphere():
    """generate_mesh of an analytic sphere against icosphere(3) of the same radius.  A mesh inscribed in the sphere stays within its
    sagitta of it, eps = r - sqrt(r^2 - e_max^2 / 3) for the longest edge e_max (the circumradius of a face is at most
    e_max / sqrt(3)); the distance between the two surfaces is at most the sum."""
    from multiply_amd import mesh, metrics
    r = 0.5
    corners = torch.tensor([[x, y, z] for x in (-r, r) for y in (-r, r) for z in (-r, r)], device="cuda")
    pred = mesh.generate_mesh(lambda x: x.norm(dim=1) - r, corners, 0.0, res_init=16, res_up=1)
    gv, gf = S.icosphere(3, radius=r, base=20)

    def sagitta(v, f):
        fv = np.asarray(v, np.float64)[np.asarray(f)]
        e = max(np.linalg.norm(fv[:, i] - fv[:, (i + 1) % 3], axis=1).max() for i in range(3))
        return r - np.sqrt(r * r - e * e / 3.0)
    eps_p, eps_g = sagitta(pred.vertices, pred.faces), sagitta(gv, gf)
    m = metrics.mesh_metrics(pred, (gv, gf), n_samples=N, seed=0)
    bound = eps_p + eps_g + TOL.delta(TOL.coordinate_scale(pred.vertices, gv))
    print(f"[sphere] {pred.faces.shape[0]} extracted faces, eps {eps_p:.3e} + {eps_g:.3e}; accuracy {m['accuracy']:.3e} completeness "
          f"{m['completeness']:.3e} (bound {bound:.3e}) normal consistency {m['normal_consistency']:.5f}")
    assert m["accuracy"] <= bound and m["completeness"] <= bound
    assert m["normal_consistency"] > TOL.NORMAL_CONSISTENCY_SPHERE


def test_volume_iou_of_offset_cubes_is_the_hand_count_and_open_meshes_are_refused():
    """the boxes and the count of tests/test_mesh_metrics_cpu.py: 120 + 120 - 48 lattice points in the union, 48 in both"""
    from multiply_amd import metrics
    a, b = S.box([0, 0, 0], [1, 1, 1]), S.box([0.5, 0.3, 0], [1.5, 1.3, 1])
    assert metrics.volume_iou(a, b, 6) == 0.25
    assert metrics.volume_iou(a, a, 5) == 1.0 and metrics.volume_iou(a, S.box([2, 0.3, 0], [3, 1.3, 1]), 9) == 0.0
    assert metrics.mesh_metrics(a, b, n_samples=64, iou_resolution=6)["volume_iou"] == 0.25
    lid_off = (a[0], a[1][:-2])
    with pytest.raises(ValueError, match="closed"):
        metrics.volume_iou(a, lid_off, 7)
    with pytest.raises(ValueError, match="closed"):
        metrics.mesh_metrics(S.unit_square(0.0), a, n_samples=64, iou_resolution=7)
    assert "volume_iou" not in metrics.mesh_metrics(S.unit_square(0.0), a, n_samples=64)        # open meshes are fine without it


def test_eval_tool_prints_the_dict_as_one_json_line(tmp_path, capsys):
    import importlib.util
    import json
    import os
    from multiply_amd import metrics
    from multiply_amd.mesh import ExtractedMesh
    pred, gt = _pair()
    paths = [ExtractedMesh(torch.from_numpy(v), torch.from_numpy(f)).export(str(tmp_path / n)) for (v, f), n in ((pred, "p.ply"), (gt, "g.ply"))]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_meshes", os.path.join(repo, "tools", "eval_meshes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(paths + ["--samples", "512", "--thresholds", "0.01", "--iou-res", "8", "--scale", "100"])
    line = capsys.readouterr().out.strip().splitlines()
    assert len(line) == 1
    assert json.loads(line[0]) == metrics.mesh_metrics(pred, gt, n_samples=512, thresholds=[0.01], unit_scale=100.0, iou_resolution=8)
