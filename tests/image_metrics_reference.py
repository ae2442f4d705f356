"""Float64 numpy restatement of the image metrics (the definitions of multiply_amd/image_metrics.py's docstring), written from
the definitions and not from the kernels: the direct 2-D window over every position, moments about the window's own mean, no
separability, no tiling, no pivot.  Inputs are converted to float64 exactly (they are float32 or uint8 / 255 in float32)."""
import numpy as np

WIN, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03


def taps():
    k = np.arange(WIN, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * SIGMA ** 2))
    return g / g.sum()


def window():
    g = taps()
    return np.outer(g, g)


def as_images(x):
    """(N, H, W, C) float32: uint8 / 255 in float32 as the module does on the host; (H, W, C) is one frame"""
    x = np.asarray(x)
    if x.ndim == 3:
        x = x[None]
    if x.dtype == np.uint8:
        x = x.astype(np.float32) / np.float32(255.0)
    assert x.dtype == np.float32 and x.ndim == 4, (x.dtype, x.shape)
    return x


def quantise_as_saved(x):
    """floor(clamp(x, 0, 1) * 255) / 255, every step in float32 (the reference's arrays are float32 when it writes its PNGs)"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        q = np.floor(np.clip(x, np.float32(0), np.float32(1)) * np.float32(255))
    return (q / np.float32(255)).astype(np.float32)


def ssim_map(a, b, data_range=1.0):
    """(N, H-10, W-10, C) float64; NaN where the window holds a non-finite value of a or b"""
    a, b = as_images(a).astype(np.float64), as_images(b).astype(np.float64)
    N, H, W, C = a.shape
    if H < WIN or W < WIN:
        raise ValueError("SSIM needs 11 x 11 pixels")
    L = float(np.float32(data_range))
    C1, C2 = (K1 * L) ** 2, (K2 * L) ** 2
    w = window()
    out = np.full((N, H - 10, W - 10, C), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            for y in range(H - 10):
                for x in range(W - 10):
                    wa, wb = a[n, y:y + WIN, x:x + WIN, :], b[n, y:y + WIN, x:x + WIN, :]        # (11, 11, C)
                    ok = np.isfinite(wa).all((0, 1)) & np.isfinite(wb).all((0, 1))
                    ww = w[:, :, None]
                    mua, mub = (ww * wa).sum((0, 1)), (ww * wb).sum((0, 1))
                    va, vb = (ww * (wa - mua) ** 2).sum((0, 1)), (ww * (wb - mub) ** 2).sum((0, 1))
                    cab = (ww * ((wa - mua) * (wb - mub))).sum((0, 1))      # as var: a == b gives cov == var, SSIM exactly 1
                    s = (2 * mua * mub + C1) * (2 * cab + C2) / ((mua ** 2 + mub ** 2 + C1) * (va + vb + C2))
                    out[n, y, x, :] = np.where(ok, s, np.nan)
    return out


def _div(num, den):
    return num / den if den > 0 else float("nan")


def ssim(a, b, mask=None, data_range=1.0):
    """dict of per-frame lists: ssim, ssim_masked, n_windows, n_masked_windows, n_left_out_windows, sums; and the map"""
    m = ssim_map(a, b, data_range)
    N, OH, OW, C = m.shape
    centre = np.ones((N, OH, OW), bool) if mask is None else np.asarray(mask, bool).reshape(N, OH + 10, OW + 10)[:, 5:5 + OH, 5:5 + OW]
    out = dict(ssim=[], ssim_masked=[], n_windows=[], n_masked_windows=[], n_left_out_windows=[], sum=[], masked_sum=[], map=m)
    for n in range(N):
        ok = ~np.isnan(m[n])
        inm = ok & centre[n][:, :, None]
        s, sm = float(m[n][ok].sum()), float(m[n][inm].sum())
        out["sum"].append(s); out["masked_sum"].append(sm)
        out["n_windows"].append(int(ok.sum())); out["n_masked_windows"].append(int(inm.sum()))
        out["n_left_out_windows"].append(int((~ok).sum()))
        out["ssim"].append(_div(s, ok.sum())); out["ssim_masked"].append(_div(sm, inm.sum()))
    return out


def psnr_of(sq_sum, count, data_range=1.0):
    L = float(np.float32(data_range))
    if count == 0:
        return float("nan")
    mse = sq_sum / count
    return float("inf") if mse == 0 else float(-10.0 * np.log10(mse / (L * L)))


def sqerr(a, b, mask=None, data_range=1.0):
    """dict of per-frame lists: sum, n_values, masked_sum, n_masked_values, n_left_out_pixels (values), psnr, psnr_masked"""
    a, b = as_images(a).astype(np.float64), as_images(b).astype(np.float64)
    N, H, W, C = a.shape
    inside = np.ones((N, H, W), bool) if mask is None else np.asarray(mask, bool).reshape(N, H, W)
    out = dict(sum=[], n_values=[], masked_sum=[], n_masked_values=[], n_left_out_pixels=[], psnr=[], psnr_masked=[])
    for n in range(N):
        ok = np.isfinite(a[n]) & np.isfinite(b[n])
        inm = ok & inside[n][:, :, None]
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (a[n] - b[n]) ** 2
        s, sm = float(d2[ok].sum()), float(d2[inm].sum())
        out["sum"].append(s); out["masked_sum"].append(sm)
        out["n_values"].append(int(ok.sum())); out["n_masked_values"].append(int(inm.sum()))
        out["n_left_out_pixels"].append(int((~ok).sum()))
        out["psnr"].append(psnr_of(s, ok.sum(), data_range)); out["psnr_masked"].append(psnr_of(sm, inm.sum(), data_range))
    return out


def nanmean(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


def image_metrics(pred, gt, mask=None, data_range=1.0, as_saved=False):
    pred, gt = as_images(pred), as_images(gt)
    if as_saved:
        pred = quantise_as_saved(pred)
    q, s = sqerr(pred, gt, mask, data_range), ssim(pred, gt, mask, data_range)
    out = dict(psnr=q["psnr"], psnr_masked=q["psnr_masked"], ssim=s["ssim"], ssim_masked=s["ssim_masked"],
               n_values=q["n_values"], n_masked_values=q["n_masked_values"], n_windows=s["n_windows"],
               n_masked_windows=s["n_masked_windows"], n_left_out_pixels=int(sum(q["n_left_out_pixels"])),
               n_left_out_windows=int(sum(s["n_left_out_windows"])), n_frames=pred.shape[0])
    for k in ("psnr", "ssim", "psnr_masked", "ssim_masked"):
        out["mean_" + k] = nanmean(out[k])
    return out


def _safe(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def scores(tp, n_pred, n_gt):
    p, r = _safe(tp, n_pred), _safe(tp, n_gt)
    return dict(iou=_safe(tp, n_pred + n_gt - tp), precision=p, recall=r, f1=_safe(2 * p * r, p + r))


def mask_metrics(pred, gt, threshold=0.5):
    """pred, gt (N, P, H, W); pred bool or opacities cut with >= threshold.  Per person (N, P), pooled (N,), sequence means."""
    pred, gt = np.asarray(pred), np.asarray(gt, bool)
    if pred.dtype != bool:
        pred = pred >= threshold
    tp, n_pred, n_gt = (pred & gt).sum((2, 3)), pred.sum((2, 3)), gt.sum((2, 3))
    out = dict(tp=tp, n_pred=n_pred, n_gt=n_gt, **scores(tp, n_pred, n_gt))
    pooled = scores(tp.sum(1), n_pred.sum(1), n_gt.sum(1))
    out.update({k + "_pooled": v for k, v in pooled.items()})
    for k in ("iou", "precision", "recall", "f1"):
        out["mean_" + k] = out[k].mean(0)
        out["mean_" + k + "_pooled"] = float(out[k + "_pooled"].mean())
    return out
