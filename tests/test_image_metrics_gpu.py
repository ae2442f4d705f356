"""The image-metric kernels (csrc/image_metrics.hip: mp_image_ssim, mp_image_sqerr) against the float64 reference
(tests/image_metrics_reference.py), and multiply_amd/image_metrics.py and tools/eval_images.py end to end.

Bounds, derived and not measured: the kernels work in double on float32 inputs, so they differ from the reference by summation
order, contraction and the pivot only -- a few 1e-16 per operation, a few hundred operations per window:
  REL  = 1e-12   relative, on the per-frame SSIM means and squared-error sums (counts are exact);
  MAP  = 2^-23   absolute, on the stored map: it lies in [-1, 1] and is rounded ONCE to float32 (half an ulp <= 2^-25).
Every test prints what it measured (pytest -s)."""
import ctypes
import json
import math
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import image_metrics_cases as K
from tests import image_metrics_reference as R
from tests.util import t32

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, MAP = 1e-12, 2.0 ** -23


def _T():
    from multiply_amd import hip
    return hip.SSIM_TILE


def shapes():
    T = _T()
    return [(1, 11, 11, 1), (1, 11, 12, 3), (1, 12, 11, 3), (1, T + 10, T + 10, 3), (1, T + 11, T + 9, 3), (3, 53, 47, 3),
            (2, 23, 47, 1)]


SHAPE_IDS = ["one window C1", "1x2 windows", "2x1 windows", "one tile", "tile+1 x tile-1", "three frames", "two frames C1"]


def raw(a, b, mask=None, data_range=1.0, want_map=True, guard=2, fill=-7.0):
    """the two C entry points on device tensors with GUARD rows behind every output: dict(ssim (N,5), sqerr (N,5), map, and the
    guard rows, which must come back untouched)"""
    from multiply_amd import hip
    L = hip.lib()
    N, H, W, C = a.shape
    m = None if mask is None else mask.contiguous().view(torch.uint8)
    out_s = torch.full((N + guard, 5), fill, dtype=torch.float64, device="cuda")
    out_q = torch.full((N + guard, 5), fill, dtype=torch.float64, device="cuda")
    smap = torch.full((N + guard, H - 10, W - 10, C), fill, dtype=torch.float32, device="cuda") if want_map else None
    nwork = int(L.mp_image_work_bytes(N, H, W, C)) // 8
    work = torch.full((nwork + 16,), fill, dtype=torch.float64, device="cuda")
    L.mp_image_ssim(a, b, m, N, H, W, C, data_range, work, out_s, smap, hip.stream())
    work_guard_s = work[nwork:].clone()
    L.mp_image_sqerr(a, b, m, N, H, W, C, work, out_q, hip.stream())
    torch.cuda.synchronize()
    guards = [out_s[N:], out_q[N:], work_guard_s, work[nwork:]] + ([smap[N:]] if want_map else [])
    return dict(ssim=out_s[:N], sqerr=out_q[:N], map=None if smap is None else smap[:N], guards=guards, fill=fill)


def guards_untouched(r):
    return all(bool((g == r["fill"]).all()) for g in r["guards"])


def same_bits(x, y):
    if x.dtype == torch.float64:
        return torch.equal(x.contiguous().view(torch.int64), y.contiguous().view(torch.int64))
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), np.finfo(np.float64).tiny)))


def compare(r, a, b, mask=None, data_range=1.0, what=""):
    """device sums / map of raw() against the reference: counts exactly, sums and means within REL, the map within MAP with its
    NaNs in the reference's places.  Returns the measured (mean rel, sum rel, map abs) errors."""
    ws, wq = R.ssim(a, b, mask, data_range), R.sqerr(a, b, mask, data_range)
    gs, gq = r["ssim"].cpu().numpy(), r["sqerr"].cpu().numpy()
    assert gs[:, 1].tolist() == ws["n_windows"] and gs[:, 3].tolist() == ws["n_masked_windows"], what
    assert gs[:, 4].tolist() == ws["n_left_out_windows"], what
    assert gq[:, 1].tolist() == wq["n_values"] and gq[:, 3].tolist() == wq["n_masked_values"], what
    assert gq[:, 4].tolist() == wq["n_left_out_pixels"], what
    e_mean = 0.0
    for col, cnt, key in ((0, 1, "ssim"), (2, 3, "ssim_masked")):
        for n in range(gs.shape[0]):
            if gs[n, cnt] > 0:
                e_mean = max(e_mean, rel(gs[n, col] / gs[n, cnt], ws[key][n]))
            else:
                assert math.isnan(ws[key][n]) and gs[n, col] == 0.0, what
    e_sum = 0.0
    for col, key in ((0, "sum"), (2, "masked_sum")):
        for n in range(gq.shape[0]):
            if wq[key][n] == 0.0:
                assert gq[n, col] == 0.0, what                             # a sum of zeros is zero
            else:
                e_sum = max(e_sum, rel(gq[n, col], wq[key][n]))
    e_map = 0.0
    if r["map"] is not None:
        gm = r["map"].cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(gm), np.isnan(ws["map"])), what
        ok = ~np.isnan(gm)
        e_map = float(np.abs(gm[ok] - ws["map"][ok]).max()) if ok.any() else 0.0
    print(f"{what}: ssim mean rel {e_mean:.2e}  sq-err sum rel {e_sum:.2e}  map abs {e_map:.2e}")
    assert e_mean <= REL and e_sum <= REL and e_map <= MAP, (what, e_mean, e_sum, e_map)
    assert guards_untouched(r), what
    return e_mean, e_sum, e_map


@lru_cache(maxsize=None)
def case(shape, content):
    a, b = K.pair(content, shape)
    return a, b, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


@pytest.mark.parametrize("content", K.CONTENTS)
@pytest.mark.parametrize("shape_id", range(7), ids=SHAPE_IDS)
def test_kernels_match_the_reference(shape_id, content):
    shape = shapes()[shape_id]
    a, b, da, db = case(shape, content)
    compare(raw(da, db), a, b, what=f"{shape} {content}")


def test_three_frames_are_three_different_answers():
    """a wrong frame stride would repeat or mix frames: the three frames' references differ far beyond the bound"""
    shape = shapes()[5]
    for content in ("noise", "ramp", "const"):
        a, b, _, _ = case(shape, content)
        s = R.ssim(a, b)["ssim"]
        q = R.sqerr(a, b)["sum"]
        assert min(abs(s[i] - s[j]) for i in range(3) for j in range(i)) > 1e-6 * max(map(abs, s)), content
        assert min(abs(q[i] - q[j]) for i in range(3) for j in range(i)) > 1e-6 * max(q), content


@pytest.mark.parametrize("content", ["noise", "flat", "ramp", "const"])
def test_swapped_arguments_and_repeated_runs_return_equal_bits(content):
    shape = shapes()[5]
    m = K.random_mask(shape)
    assert all(f.any() and not f.all() for f in m)                         # per frame, on the host, before the device is touched
    _, _, da, db = case(shape, content)
    mask = torch.from_numpy(m).cuda()
    r1, r2, rs = raw(da, db, mask), raw(da, db, mask), raw(db, da, mask)
    for k in ("ssim", "sqerr", "map"):
        assert same_bits(r1[k], r2[k]), ("two runs", k)
        assert same_bits(r1[k], rs[k]), ("swapped", k)
    ident = raw(da, da)
    assert bool((ident["map"] == 1.0).all()) and ident["ssim"][:, 0].tolist() == ident["ssim"][:, 1].tolist()
    assert ident["sqerr"][:, 0].tolist() == [0.0] * 3


def test_data_range_scales_the_constants():
    shape = (1, 20, 19, 3)
    a, b = K.pair("8bit", shape)
    a255, b255 = (a * np.float32(255)).round().astype(np.float32), (b * np.float32(255)).round().astype(np.float32)
    r = raw(torch.from_numpy(a255).cuda(), torch.from_numpy(b255).cuda(), data_range=255.0)
    compare(r, a255, b255, data_range=255.0, what="data_range 255")
    from multiply_amd import image_metrics as IM
    got, want = IM.image_metrics(a255, b255, data_range=255.0), R.image_metrics(a255, b255, data_range=255.0)
    assert rel(got["psnr"], want["psnr"]) <= REL and rel(got["ssim"], want["ssim"]) <= REL
    assert abs(got["psnr"][0] - R.image_metrics(a, b)["psnr"][0]) < 1e-5         # the same frames in [0, 1]


def _one_pixel(shape, n, y, x):
    m = np.zeros(shape[:3], bool)
    m[n, y, x] = True
    return m


def test_masks():
    from multiply_amd import image_metrics as IM
    shape = shapes()[5]
    N, H, W, C = shape
    T = _T()
    masks = {"random": K.random_mask(shape),
             "one pixel, a window centre on a tile corner": _one_pixel(shape, 1, T - 1 + 5, T + 5),
             "one pixel, the first window centre": _one_pixel(shape, 0, 5, 5),
             "one pixel, the last window centre": _one_pixel(shape, 2, H - 6, W - 6),
             "one pixel in the border, no window's centre": _one_pixel(shape, 2, 4, 20),
             "one pixel, the image's last": _one_pixel(shape, 0, H - 1, W - 1)}
    for name, m in masks.items():
        assert m.any() and not m.all(), name                               # on the host, before the device is touched
    full, empty = np.ones(shape[:3], bool), np.zeros(shape[:3], bool)
    assert full.all() and not empty.any()
    a, b, da, db = case(shape, "noise")
    plain = raw(da, db)
    for name, m in masks.items():
        compare(raw(da, db, torch.from_numpy(m).cuda()), a, b, m, what=name)
    rf = raw(da, db, torch.from_numpy(full).cuda())
    assert same_bits(rf["ssim"], plain["ssim"]) and same_bits(rf["sqerr"], plain["sqerr"]) and same_bits(rf["map"], plain["map"])
    assert same_bits(rf["ssim"][:, 2:4], rf["ssim"][:, 0:2]) and same_bits(rf["sqerr"][:, 2:4], rf["sqerr"][:, 0:2])
    re_ = raw(da, db, torch.from_numpy(empty).cuda())
    assert re_["ssim"][:, 2:4].abs().sum() == 0 and re_["sqerr"][:, 2:4].abs().sum() == 0
    assert same_bits(re_["ssim"][:, :2], plain["ssim"][:, :2])
    got = IM.image_metrics(a, b, mask=empty)
    assert np.isnan(got["psnr_masked"]).all() and np.isnan(got["ssim_masked"]).all() and math.isnan(got["mean_ssim_masked"])
    assert got["n_masked_values"].tolist() == [0] * N and got["n_masked_windows"].tolist() == [0] * N
    assert rel(got["ssim"], R.ssim(a, b)["ssim"]) <= REL
    border = IM.image_metrics(a, b, mask=masks["one pixel in the border, no window's centre"])
    assert border["n_masked_windows"].tolist() == [0, 0, 0] and border["n_masked_values"].tolist() == [0, 0, C]
    assert np.isnan(border["ssim_masked"]).all() and np.isfinite(border["psnr_masked"][2]) and np.isnan(border["psnr_masked"][:2]).all()


def test_non_finite_values_are_left_out_and_counted():
    shape = shapes()[5]
    N, H, W, C = shape
    T = _T()
    a, b = (x.copy() for x in K.pair("noise", shape))
    a[0, T - 1 + 5, T + 5, 1] = np.nan             # the centre of the window on the corner of four tiles
    a[0, 0, 0, 0] = np.nan                         # the tile's pivot pixel: one window
    b[1, 20, 21, 0] = np.inf
    a[1, 20, 21, 0] = np.inf                       # inf - inf
    a[1, T + 4, 3, 2] = -np.inf                    # a pixel in the halo two tiles share
    b[2, H - 1, W - 1, 2] = np.nan                 # the last pixel: one window
    a[2, 30, 30, :] = np.nan                       # all channels of one pixel
    b[2, 30, 31, 1] = np.nan                       # the neighbour: the windows overlap, each is left out once
    m = K.random_mask(shape)
    assert all(f.any() and not f.all() for f in m)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = R.ssim(a, b)
    # by hand: 11 x 10 windows hold pixel (36, 37) of a 47-pixel-wide image, 1 the corner; 121 the inf, 11 x 4 pixel (36, 3);
    # 1 the last pixel, 3 x 121 the NaN pixel, 11 more the column its neighbour adds in channel 1
    assert want["n_left_out_windows"] == [110 + 1, 121 + 44, 1 + 3 * 121 + 11] and R.sqerr(a, b)["n_left_out_pixels"] == [2, 2, 5]
    compare(raw(da, db), a, b, what="non-finite")
    compare(raw(da, db, torch.from_numpy(m).cuda()), a, b, m, what="non-finite, masked")
    from multiply_amd import image_metrics as IM
    got = IM.image_metrics(a, b)
    assert got["n_left_out_pixels"] == 9 and got["n_left_out_windows"] == sum(want["n_left_out_windows"])
    assert np.isfinite(got["psnr"]).all() and np.isfinite(got["ssim"]).all()
    # a single-frame image whose every window holds a NaN: nothing counted, NaN, not an error
    c = np.full((1, 12, 12, 1), 0.5, np.float32)
    c[0, 5:7, 5:7, 0] = np.nan
    lone = IM.image_metrics(c, c)
    assert lone["n_windows"].tolist() == [0] and math.isnan(lone["ssim"][0]) and lone["n_left_out_windows"] == 4
    assert lone["psnr"][0] == np.inf and lone["n_left_out_pixels"] == 4 and math.isnan(lone["mean_ssim"])


def test_null_map_zero_frames_and_status_codes():
    from multiply_amd import hip
    hip.require_device()
    shape = shapes()[4]
    a, b, da, db = case(shape, "flat")
    with_map, without = raw(da, db), raw(da, db, want_map=False)
    assert without["map"] is None and same_bits(with_map["ssim"], without["ssim"]) and guards_untouched(without)
    N, H, W, C = shape
    lib = ctypes.CDLL(hip.LIB_PATH)                                        # no errcheck: the status itself
    for name, (rt, at) in hip.header_prototypes().items():
        if name.startswith("mp_image_"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = rt, at
    out = torch.full((2, 5), -7.0, dtype=torch.float64, device="cuda")
    work = torch.full((int(lib.mp_image_work_bytes(N, H, W, C)) // 8,), -7.0, dtype=torch.float64, device="cuda")
    smap = torch.full((1, H - 10, W - 10, C), -7.0, device="cuda")
    st = hip.stream()
    assert lib.mp_image_ssim(da, db, None, 0, H, W, C, 1.0, work, out, smap, st) == 0          # N == 0: a no-op
    assert lib.mp_image_sqerr(da, db, None, 0, H, W, C, work, out, st) == 0
    assert lib.mp_image_ssim(None, None, None, 0, H, W, C, 1.0, None, None, None, st) == 0
    for bad in (dict(N=-1), dict(H=10), dict(W=10), dict(C=2), dict(L=0.0), dict(L=float("nan")), dict(a=None), dict(b=None),
                dict(work=None), dict(out=None)):
        k = dict(a=da, b=db, N=1, H=H, W=W, C=C, L=1.0, work=work, out=out)
        k.update(bad)
        assert lib.mp_image_ssim(k["a"], k["b"], None, k["N"], k["H"], k["W"], k["C"], k["L"], k["work"], k["out"], smap, st) == -1, bad
        if "L" not in bad and bad not in (dict(H=10), dict(W=10)):
            assert lib.mp_image_sqerr(k["a"], k["b"], None, k["N"], k["H"], k["W"], k["C"], k["work"], k["out"], st) == -1, bad
    assert lib.mp_image_sqerr(da, db, None, 1, 0, W, C, work, out, st) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((work == -7).all()) and bool((smap == -7).all())   # nothing was launched
    with pytest.raises(RuntimeError, match="mp_image_ssim failed with code -1"):               # the binding raises on it
        hip.lib().mp_image_ssim(da, db, None, 1, 10, W, C, 1.0, work, out, None, st)
    empty = torch.empty(0, 12, 12, 3, device="cuda")
    o, m = hip.image_ssim(empty, empty, want_map=True)
    assert o.shape == (0, 5) and m.shape == (0, 2, 2, 3) and hip.image_sqerr(empty, empty).shape == (0, 5)
    # a 10-row image has a PSNR and no SSIM
    from multiply_amd import image_metrics as IM
    small = K.pair("noise", (2, 10, 9, 3))
    assert rel(IM.psnr(*small), R.sqerr(*small)["psnr"]) <= REL
    with pytest.raises(ValueError):
        IM.ssim(*small)


def _close(got, want, what):
    for k, w in want.items():
        g = got[k]
        if isinstance(w, (list, np.ndarray)):
            g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (what, k)
            ok = np.isfinite(w)
            assert not ok.any() or rel(g[ok], w[ok]) <= REL, (what, k, g, w)
        elif isinstance(w, float) and not math.isfinite(w):
            assert (math.isnan(w) and math.isnan(g)) or g == w, (what, k)
        else:
            assert g == w if isinstance(w, int) else rel(g, w) <= REL, (what, k, g, w)


def test_image_metrics_end_to_end():
    """host arrays, device tensors and uint8 frames; masked; as_saved"""
    from multiply_amd import image_metrics as IM
    shape = shapes()[5]
    m = K.random_mask(shape)
    assert all(f.any() and not f.all() for f in m)
    a, b, da, db = case(shape, "flat")
    _close(IM.image_metrics(a, b, mask=m), R.image_metrics(a, b, mask=m), "numpy")
    det = {}
    _close(IM.image_metrics(da, torch.from_numpy(b), mask=torch.from_numpy(m), details=det), R.image_metrics(a, b, mask=m), "tensors")
    assert det["ssim_map"].shape == (3, 43, 37, 3) and det["ssim"].shape == (3, 5) and det["sqerr"].dtype == torch.float64
    n8, m8 = K.pair("noise", shape)
    u8 = (m8 * 255).astype(np.uint8)
    _close(IM.image_metrics(n8, u8), R.image_metrics(n8, u8), "uint8 ground truth")
    _close(IM.image_metrics(n8 * 1.2 - 0.1, u8, as_saved=True), R.image_metrics(n8 * np.float32(1.2) - np.float32(0.1), u8, as_saved=True),
           "as_saved")
    saved = (np.clip(n8, 0, 1) * 255).astype(np.uint8)                      # scoring the saved file gives the same numbers
    _close(IM.image_metrics(n8, u8, as_saved=True), R.image_metrics(saved, u8), "as_saved = the saved file")
    assert rel(IM.psnr(a, b, mask=m), R.image_metrics(a, b, mask=m)["psnr_masked"]) <= REL
    assert rel(IM.ssim(a, b), R.image_metrics(a, b)["ssim"]) <= REL
    one = IM.image_metrics(a[0], b[0])                                     # (H, W, C): one frame
    assert one["n_frames"] == 1 and rel(one["ssim"], R.image_metrics(a[:1], b[:1])["ssim"]) <= REL


def test_mask_metrics_on_the_device():
    from multiply_amd import image_metrics as IM
    g = np.random.default_rng(3)
    soft = g.random((3, 2, 17, 19)).astype(np.float32)
    soft[0, 1] = 0.0                                                       # an empty prediction
    gt = g.random((3, 2, 17, 19)) < 0.4
    gt[1, 0] = False                                                       # an empty ground truth
    for pred in (soft, soft >= 0.5):
        got = IM.mask_metrics(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())
        want = R.mask_metrics(pred, gt)
        for k, w in want.items():
            assert np.allclose(got[k], w, rtol=0, atol=1e-15), k
    assert got["iou"][0, 1] == 0.0 and got["recall"][1, 0] == 0.0
    lo = IM.mask_metrics(torch.from_numpy(soft).cuda(), torch.from_numpy(gt).cuda(), threshold=0.25)
    assert np.array_equal(lo["n_pred"], (soft >= 0.25).sum((2, 3)))


@pytest.fixture(scope="module")
def render():
    """one 24 x 24 eval render of the seeded one-person model, left unchanged"""
    import warnings
    warnings.filterwarnings("ignore")
    from multiply_amd.config import load_config
    from multiply_amd.multiply import Multiply
    from multiply_amd.synthetic import make_scene, make_smpl_tables
    sc = make_scene(1, seed=2, H=24, W=24)
    torch.manual_seed(0)
    model = Multiply(load_config(), sc["smpl_params"][0, 0, 76:], smpl_tables=make_smpl_tables(0)).eval()
    sp = t32(sc["smpl_params"])
    inp = dict(uv=t32(sc["uv"]), intrinsics=t32(sc["intrinsics"]), pose=t32(sc["pose"]), smpl_params=sp,
               smpl_pose=sp[:, :, 4:76], smpl_shape=sp[:, :, 76:], smpl_trans=sp[:, :, 1:4], idx=torch.tensor([1]))
    out = model({k: v.cuda() for k, v in inp.items()})
    torch.cuda.synchronize()
    return {k: out[k].detach().clone() for k in ("rgb_values", "acc_person_list")}


def test_frame_metrics_on_an_eval_render(render):
    from multiply_amd import image_metrics as IM
    H = W = 24
    rgb = render["rgb_values"].cpu().numpy().reshape(H, W, 3)
    acc = render["acc_person_list"].cpu().numpy().reshape(H, W, 1).transpose(2, 0, 1)
    n_bad = int((~np.isfinite(rgb)).sum())
    own = IM.frame_metrics(render, {"rgb": render["rgb_values"]}, (H, W), gt_masks=torch.from_numpy(acc >= 0.5))
    im, mk = own["image"], own["masks"]
    assert im["n_left_out_pixels"] == n_bad and im["n_values"][0] == H * W * 3 - n_bad
    if im["n_windows"][0]:
        assert im["ssim"][0] == 1.0 and im["mean_ssim"] == 1.0
    assert im["psnr"][0] == np.inf and im["mean_psnr"] == np.inf
    person = int((acc >= 0.5).sum())
    assert mk["tp"].tolist() == [[person]] and mk["n_pred"].tolist() == [[person]]
    assert mk["iou"].tolist() == [[1.0 if person else 0.0]] and mk["f1_pooled"].tolist() == [1.0 if person else 0.0]
    # a copy shifted by one pixel along x (and the masks with it) against the reference
    shifted = np.ascontiguousarray(np.roll(rgb, 1, axis=1))
    gt_mask = np.roll(acc >= 0.5, 1, axis=1)
    got = IM.frame_metrics(render, shifted.reshape(-1, 3), (H, W), gt_masks=gt_mask, mask=gt_mask[0])
    _close(got["image"], R.image_metrics(rgb[None], shifted[None], mask=gt_mask), "shifted render")
    want = R.mask_metrics((acc >= 0.5)[None], gt_mask[None])
    for k, w in want.items():
        assert np.allclose(got["masks"][k], w, rtol=0, atol=1e-15), k
    print(f"render: {n_bad} non-finite values, person pixels {person}, shifted psnr {got['image']['psnr'][0]:.3f} "
          f"ssim {got['image']['ssim'][0]:.6f} iou {got['masks']['iou'][0, 0]:.4f}")
    with pytest.raises(ValueError):
        IM.frame_metrics(render, shifted, (H, W + 1))


def test_eval_images_tool_on_a_folder_of_pngs(tmp_path):
    from PIL import Image
    from multiply_amd import image_metrics as IM
    g = np.random.default_rng(5)
    pred = (g.random((3, 24, 20, 3)) * 255).astype(np.uint8)
    gt = np.clip(pred.astype(np.int64) + g.integers(-20, 21, pred.shape), 0, 255).astype(np.uint8)
    mask = g.random((3, 24, 20)) < 0.5
    assert all(f.any() and not f.all() for f in mask)
    pm, gm = g.random((3, 2, 24, 20)) < 0.5, g.random((3, 2, 24, 20)) < 0.5
    for i in range(3):
        for d, img in (("pred", pred[i]), ("gt", gt[i]), ("mask", (mask[i] * 255).astype(np.uint8))):
            os.makedirs(tmp_path / d, exist_ok=True)
            Image.fromarray(img).save(tmp_path / d / f"{i:04d}.png")
        for p in range(2):
            for d, img in (("pm", pm[i, p]), ("gm", gm[i, p])):
                os.makedirs(tmp_path / d / str(p), exist_ok=True)
                Image.fromarray((img * 255).astype(np.uint8)).save(tmp_path / d / str(p) / f"{i:04d}.png")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "eval_images.py"), str(tmp_path / "pred"), str(tmp_path / "gt"),
                        "--mask-dir", str(tmp_path / "mask"), "--pred-mask-dir", str(tmp_path / "pm"), "--gt-mask-dir",
                        str(tmp_path / "gm"), "--as-saved"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    got = json.loads(lines[0])
    want = IM.image_metrics(pred, gt, mask=mask, as_saved=True)
    for k, w in want.items():
        assert got[k] == (w.tolist() if isinstance(w, np.ndarray) else w), k          # the same kernels, the same bits
    wm = IM.mask_metrics(pm, gm)
    for k, w in wm.items():
        assert got["masks"][k] == (w.tolist() if isinstance(w, np.ndarray) else w), k
    _close(want, R.image_metrics(pred, gt, mask=mask, as_saved=True), "the tool's numbers")
