"""The float64 reference of the image metrics (tests/image_metrics_reference.py) on analytic anchors, and the host code of
multiply_amd/image_metrics.py that needs no device: the accepted inputs, the quantisation, the mask scores, the header's new
entry points, the command-line tool's arguments."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import image_metrics_cases as K
from tests import image_metrics_reference as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_taps_sum_to_one_and_are_symmetric():
    g = R.taps()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[5] / g[4] - np.exp(1.0 / 4.5)) < 1e-15                    # exp(-(k-5)^2 / (2 1.5^2))
    w = R.window()
    assert w.shape == (11, 11) and abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w.T)


def test_identical_images_give_ssim_one_and_infinite_psnr():
    a, _ = K.pair("noise", (2, 13, 14, 3))
    s, q = R.ssim(a, a), R.sqerr(a, a)
    assert np.array_equal(s["map"], np.ones((2, 3, 4, 3))) and s["ssim"] == [1.0, 1.0]
    assert q["psnr"] == [float("inf")] * 2 and q["sum"] == [0.0, 0.0] and q["n_values"] == [13 * 14 * 3] * 2
    m = R.image_metrics(a, a)
    assert m["mean_ssim"] == 1.0 and m["mean_psnr"] == float("inf") and m["n_left_out_pixels"] == 0 and m["n_left_out_windows"] == 0


def test_two_constant_images():
    """every map value is (2ab + C1) / (a^2 + b^2 + C1): 0.65758115326... for 0.3 / 0.8 (the float32 nearest to 0.3 and 0.8 move
    it by 1.2e-8); PSNR = -10 log10((a - b)^2)"""
    a32, b32 = np.float32(0.3), np.float32(0.8)
    a, b = np.full((1, 12, 15, 3), a32), np.full((1, 12, 15, 3), b32)
    m = R.ssim_map(a, b)
    af, bf = float(a32), float(b32)
    want = (2 * af * bf + 1e-4) / (af * af + bf * bf + 1e-4)
    assert m.shape == (1, 2, 5, 3) and np.abs(m - want).max() < 1e-15
    assert abs((2 * 0.3 * 0.8 + 1e-4) / (0.3 ** 2 + 0.8 ** 2 + 1e-4) - 0.65758115326) < 1e-11 and abs(want - 0.65758115326) < 5e-8
    assert abs(R.sqerr(a, b)["psnr"][0] - (-10 * np.log10((af - bf) ** 2))) < 1e-13
    assert abs(R.sqerr(a, b)["psnr"][0] - (-10 * np.log10(0.25))) < 1e-6
    # data_range scales C1, C2 and the PSNR's peak: 255 x the images with data_range 255 give the same numbers
    s255 = R.ssim_map(a * np.float32(255), b * np.float32(255), 255.0)
    assert np.abs(s255 - m).max() < 1e-7
    assert abs(R.sqerr(a * np.float32(255), b * np.float32(255), data_range=255.0)["psnr"][0] - R.sqerr(a, b)["psnr"][0]) < 1e-6


def test_one_nan_leaves_out_121_windows_and_one_value():
    a, b = K.pair("noise", (1, 31, 33, 3))
    a[0, 12, 17, 1] = np.nan                                               # at least 10 from every border
    s, q = R.ssim(a, b), R.sqerr(a, b)
    assert s["n_left_out_windows"] == [121] and s["n_windows"] == [21 * 23 * 3 - 121]
    assert q["n_left_out_pixels"] == [1] and q["n_values"] == [31 * 33 * 3 - 1]
    bad = np.isnan(s["map"][0])
    assert bad[2:13, 7:18, 1].all() and bad.sum() == 121 and np.isfinite(s["ssim"][0]) and np.isfinite(q["psnr"][0])
    b[0, 0, 0, 2] = np.inf                                                 # a corner: one window
    assert R.ssim(a, b)["n_left_out_windows"] == [122] and R.sqerr(a, b)["n_left_out_pixels"] == [2]


def test_masked_variants_of_the_reference():
    shape = (2, 14, 13, 3)
    a, b = K.pair("noise", shape)
    full, empty = np.ones(shape[:3], bool), np.zeros(shape[:3], bool)
    s, q = R.ssim(a, b), R.sqerr(a, b)
    sf, qf = R.ssim(a, b, full), R.sqerr(a, b, full)
    assert sf["ssim_masked"] == s["ssim"] and qf["psnr_masked"] == q["psnr"]
    se, qe = R.ssim(a, b, empty), R.sqerr(a, b, empty)
    assert all(np.isnan(v) for v in se["ssim_masked"] + qe["psnr_masked"]) and se["n_masked_windows"] == [0, 0] and qe["n_masked_values"] == [0, 0]
    one = empty.copy()
    one[0, 6, 7] = True                                                    # the centre of window (1, 2)
    so, qo = R.ssim(a, b, one), R.sqerr(a, b, one)
    assert so["n_masked_windows"] == [3, 0] and abs(so["ssim_masked"][0] - s["map"][0, 1, 2].mean()) < 1e-15
    assert qo["n_masked_values"] == [3, 0] and abs(qo["masked_sum"][0] - ((a[0, 6, 7].astype(float) - b[0, 6, 7]) ** 2).sum()) < 1e-15
    edge = empty.copy()
    edge[1, 4, 7] = True                                                   # row 4 is no window's centre: PSNR sees it, SSIM does not
    assert R.ssim(a, b, edge)["n_masked_windows"] == [0, 0] and R.sqerr(a, b, edge)["n_masked_values"] == [0, 3]


def test_as_saved_equals_quantising_by_hand():
    from multiply_amd import image_metrics as IM
    x = np.array([-0.5, 0.0, 0.2, 0.49999, 0.5, 0.004, 0.9999, 1.0, 1.7, np.nan], np.float32)
    want = np.array([0, 0, 51, 127, 127, 1, 254, 255, 255, np.nan], np.float32) / np.float32(255)
    got = IM.quantise_as_saved(torch.from_numpy(x)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(R.quantise_as_saved(x), want, equal_nan=True)
    # ... which is what writing the uint8 image and reading it back gives
    img = torch.rand(1, 12, 12, 3, generator=torch.Generator().manual_seed(0))
    u8 = (img.numpy() * 255).astype(np.uint8)
    assert np.array_equal(IM.quantise_as_saved(img).numpy(), IM.as_images(u8).numpy())
    a, b = K.pair("noise", (1, 12, 13, 3))
    assert R.image_metrics(a, b, as_saved=True) == R.image_metrics(R.quantise_as_saved(a), b)
    assert R.image_metrics(a, b, as_saved=True)["psnr"] != R.image_metrics(a, b)["psnr"]


def test_mask_score_identities_on_a_hand_made_case():
    """4 x 4, two persons.  Person 0: pred = the left half (8), gt = the top half (8), overlap 4: IoU 4/12, P = R = F1 = 1/2.
    Person 1: pred empty, gt 2 pixels: everything 0 (zero denominators give 0).  Pooled: tp 4, pred 8, gt 10: IoU 4/14, P 1/2,
    R 2/5, F1 8/18."""
    from multiply_amd import image_metrics as IM
    pred, gt = np.zeros((1, 2, 4, 4), bool), np.zeros((1, 2, 4, 4), bool)
    pred[0, 0, :, :2] = True
    gt[0, 0, :2, :] = True
    gt[0, 1, 3, 2:] = True
    soft = np.where(pred, 0.5, 0.49999).astype(np.float32)                 # >= threshold: 0.5 is inside
    for m in (R.mask_metrics(pred, gt), IM.mask_metrics(pred, gt), IM.mask_metrics(torch.from_numpy(soft), torch.from_numpy(gt)),
              R.mask_metrics(soft, gt)):
        assert m["tp"].tolist() == [[4, 0]] and m["n_pred"].tolist() == [[8, 0]] and m["n_gt"].tolist() == [[8, 2]]
        assert np.allclose(m["iou"], [[1 / 3, 0]], atol=1e-15) and np.allclose(m["f1"], [[0.5, 0]], atol=1e-15)
        assert np.allclose(m["precision"], [[0.5, 0]], atol=1e-15) and np.allclose(m["recall"], [[0.5, 0]], atol=1e-15)
        assert abs(m["iou_pooled"][0] - 4 / 14) < 1e-15 and abs(m["precision_pooled"][0] - 0.5) < 1e-15
        assert abs(m["recall_pooled"][0] - 0.4) < 1e-15 and abs(m["f1_pooled"][0] - 8 / 18) < 1e-15
        assert abs(m["mean_iou_pooled"] - 4 / 14) < 1e-15 and np.allclose(m["mean_iou"], [1 / 3, 0], atol=1e-15)
    both_empty = IM.mask_metrics(np.zeros((2, 1, 4, 4), bool), np.zeros((2, 1, 4, 4), bool))
    assert both_empty["iou"].tolist() == [[0.0], [0.0]] and both_empty["mean_f1_pooled"] == 0.0
    with pytest.raises(ValueError):
        IM.mask_metrics(pred, gt[:, :1])
    with pytest.raises(TypeError):
        IM.mask_metrics(pred, gt.astype(np.float32))                       # the ground truth is bool


def test_module_imports_without_a_device_and_checks_its_inputs(monkeypatch):
    from multiply_amd import hip, image_metrics as IM
    for fn in ("psnr", "ssim", "image_metrics", "mask_metrics", "frame_metrics"):
        assert callable(getattr(IM, fn))
    for k in ("PSNR", "SSIM", "11 taps", "K1 = 0.01", "K2 = 0.03", "as_saved", "threshold", "non-finite"):
        assert k in IM.__doc__, k
    reached = []
    monkeypatch.setattr(hip, "require_device", lambda: reached.append(1) or (_ for _ in ()).throw(RuntimeError("device")))
    ok = np.zeros((2, 12, 12, 3), np.float32)
    with pytest.raises(ValueError, match="11 x 11"):
        IM.image_metrics(np.zeros((1, 10, 12, 3), np.float32), np.zeros((1, 10, 12, 3), np.float32))      # H = 10
    with pytest.raises(ValueError, match="11 x 11"):
        IM.ssim(np.zeros((1, 12, 10, 1), np.float32), np.zeros((1, 12, 10, 1), np.float32))
    with pytest.raises(ValueError, match="differ in shape"):
        IM.image_metrics(ok, ok[:, :, :11])
    with pytest.raises(ValueError):
        IM.image_metrics(np.zeros((2, 12, 12, 2), np.float32), np.zeros((2, 12, 12, 2), np.float32))      # C = 2
    with pytest.raises(TypeError):
        IM.image_metrics(ok.astype(np.float64), ok)
    with pytest.raises(TypeError):
        IM.psnr(ok, ok.astype(np.int32))
    with pytest.raises(TypeError, match="bool"):
        IM.image_metrics(ok, ok, mask=np.ones((2, 12, 12), np.float32))
    with pytest.raises(ValueError, match="mask"):
        IM.image_metrics(ok, ok, mask=np.ones((2, 12, 11), bool))
    assert not reached                                                     # every refusal came before the device was asked for
    with pytest.raises(RuntimeError, match="device"):
        IM.image_metrics(ok, (ok * 255).astype(np.uint8))                  # float32 against uint8 is accepted; then the device
    assert reached
    assert IM.as_images(np.full((12, 12, 3), 51, np.uint8)).shape == (1, 12, 12, 3)
    assert IM.as_images(np.full((12, 12, 3), 51, np.uint8)).unique().tolist() == [np.float32(51) / np.float32(255)]
    # the binding's own checks (hip.image_ssim / image_sqerr) refuse the same before any launch
    with pytest.raises(ValueError):
        hip.image_ssim(torch.zeros(1, 10, 12, 3), torch.zeros(1, 10, 12, 3))
    with pytest.raises(TypeError):
        hip.image_sqerr(torch.zeros(1, 12, 12, 3, dtype=torch.float64), torch.zeros(1, 12, 12, 3, dtype=torch.float64))
    assert np.isnan(IM.psnr_from_sums([0.0], [0])[0]) and IM.psnr_from_sums([0.0], [5])[0] == np.inf
    assert abs(IM.psnr_from_sums([2.5], [10])[0] - (-10 * np.log10(0.25))) < 1e-14


def test_header_declares_the_new_entry_points():
    from multiply_amd import hip
    protos = hip.header_prototypes()
    want = {"mp_image_ssim": 12, "mp_image_sqerr": 10, "mp_image_work_bytes": 4}
    for name, nargs in want.items():
        assert name in protos and protos[name][0] is ctypes.c_int and len(protos[name][1]) == nargs, name
    assert protos["mp_image_ssim"][1] == [hip.DevPtr] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] + [hip.DevPtr] * 4
    assert protos["mp_image_work_bytes"][1] == [ctypes.c_int] * 4 and "mp_image_work_bytes" in hip.VALUE_RETURNING
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    assert int(re.search(r"#define MP_SSIM_TILE (\d+)", hdr).group(1)) == hip.SSIM_TILE and hip.SSIM_WINDOW == R.WIN
    assert callable(hip.image_ssim) and callable(hip.image_sqerr)


def test_work_bytes_and_argument_errors_need_no_device():
    """mp_image_work_bytes is host arithmetic, and every -1 of the two launchers is decided before anything touches the device"""
    from multiply_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    T = 32
    assert lib.mp_image_work_bytes(0, 11, 11, 1) == 0 and lib.mp_image_work_bytes(1, 11, 11, 1) == 40
    assert lib.mp_image_work_bytes(2, T + 11, T + 9, 3) == 2 * 40 * max(2, -(-(T + 11) * (T + 9) * 3 // 4096))
    assert lib.mp_image_work_bytes(75, 512, 512, 3) == 75 * 40 * max(16 * 16, 512 * 512 * 3 // 4096)
    assert lib.mp_image_work_bytes(3, 5, 4, 3) == 3 * 40                   # too small for SSIM, fine for the squared error
    for bad in ((-1, 12, 12, 3), (1, 0, 12, 3), (1, 12, 12, 2), (1, 12, 12, 4), (1 << 20, 4096, 4096, 3)):
        assert lib.mp_image_work_bytes(*bad) == -1, bad
    lib.mp_image_ssim.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_float] + [ctypes.c_void_p] * 4
    lib.mp_image_sqerr.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    p = 0x1000                                                             # never dereferenced: each call is refused on its arguments
    for N, H, W, C, L in ((1, 10, 12, 3, 1.0), (1, 12, 10, 3, 1.0), (1, 12, 12, 2, 1.0), (-1, 12, 12, 3, 1.0), (1, 12, 12, 3, 0.0),
                          (1, 12, 12, 3, float("nan")), (1, 12, 12, 3, float("inf"))):
        assert lib.mp_image_ssim(p, p, None, N, H, W, C, L, p, p, None, None) == -1, (N, H, W, C, L)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        a, b, work, out = args
        assert lib.mp_image_ssim(a, b, None, 1, 12, 12, 3, 1.0, work, out, None, None) == -1
        assert lib.mp_image_sqerr(a, b, None, 1, 12, 12, 3, work, out, None) == -1
    assert lib.mp_image_sqerr(p, p, None, 1, 0, 12, 3, p, p, None) == -1 and lib.mp_image_sqerr(p, p, None, 1, 12, 12, 2, p, p, None) == -1
    assert lib.mp_image_sqerr(p, p, None, 1, 40000, 40000, 3, p, p, None) == -1          # H W C >= 2^31
    assert lib.mp_image_ssim(None, None, None, 0, 12, 12, 3, 1.0, None, None, None, None) == 0     # N == 0: a valid no-op
    assert lib.mp_image_sqerr(None, None, None, 0, 12, 12, 3, None, None, None) == 0


def test_eval_tool_help_runs_and_refuses_mismatched_folders(tmp_path, monkeypatch):
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_images.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "PRED_DIR GT_DIR" in r.stdout and "--as-saved" in r.stdout and "--pred-mask-dir" in r.stdout
    import importlib.util
    from PIL import Image
    spec = importlib.util.spec_from_file_location("eval_images", os.path.join(REPO, "tools", "eval_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from multiply_amd import hip, image_metrics
    monkeypatch.setattr(hip, "require_device", lambda: None)
    seen = {}
    monkeypatch.setattr(image_metrics, "image_metrics", lambda *a, **k: seen.update(a=a, k=k) or {"psnr": np.array([1.0, 2.0]), "mean_psnr": 1.5})
    g = np.random.default_rng(0)
    for d, n, size in (("pred", 2, (12, 14)), ("gt", 2, (12, 14)), ("short", 1, (12, 14)), ("small", 2, (12, 13)), ("mask", 2, (12, 14))):
        os.makedirs(tmp_path / d)
        for i in range(n):
            Image.fromarray((g.random(size + (3,)) * 255).astype(np.uint8)).save(tmp_path / d / f"{i:04d}.png")
    out = mod.main([str(tmp_path / "pred"), str(tmp_path / "gt"), "--mask-dir", str(tmp_path / "mask"), "--as-saved"])
    assert out == {"psnr": [1.0, 2.0], "mean_psnr": 1.5}
    pred, gt = seen["a"]
    assert pred.shape == gt.shape == (2, 12, 14, 3) and pred.dtype == np.uint8 and seen["k"]["as_saved"] is True
    assert seen["k"]["mask"].shape == (2, 12, 14) and seen["k"]["mask"].dtype == bool
    for other in ("short", "small"):
        with pytest.raises(SystemExit):
            mod.main([str(tmp_path / "pred"), str(tmp_path / other)])
    with pytest.raises(SystemExit):
        mod.main([str(tmp_path / "pred"), str(tmp_path / "gt"), "--pred-mask-dir", str(tmp_path / "mask")])
