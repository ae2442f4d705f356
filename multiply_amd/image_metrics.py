"""Image-space metrics: how close rendered frames are to ground-truth frames, and predicted person masks to ground-truth masks.

The method this project restates is judged on novel-view quality (PSNR, SSIM of the rendered frames) and on human segmentation
(IoU, recall, F1 of the per-person masks).  The reference project has `get_psnr` (code/lib/utils/rend_util.py:10-18) and otherwise
writes PNGs for an outside script to score, so the definitions below are the published ones, spelled out:

  images      (N, H, W, C) float32, C = 1 or 3, values in [0, data_range] (data_range = 1 by default, passed on as a float32); a
              (H, W, C) array is one frame; uint8 input is divided by 255 on the host.  A VALUE is one channel of one pixel.
  psnr        per frame, -10 log10(MSE / data_range^2), the MSE over all values of the frame (pixels and channels): for
              data_range = 1 the reference's get_psnr(normalize_rgb=False).  +inf for identical frames.
  ssim        Wang, Bovik, Sheikh, Simoncelli, Image quality assessment: from error visibility to structural similarity, IEEE TIP
              2004, in the setting everyone reports: a Gaussian window of 11 taps, sigma = 1.5 -- taps exp(-(k-5)^2 / (2 sigma^2)),
              k = 0..10, formed in double and normalised to sum 1, the 2-D window their outer product w --; K1 = 0.01, K2 = 0.03,
              C1 = (K1 L)^2, C2 = (K2 L)^2, L = data_range; per channel, with the window's weighted population (biased) moments
              mu_a = sum w a, var_a = sum w (a - mu_a)^2, cov = sum w (a - mu_a)(b - mu_b):
                  SSIM = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2)).
              The map exists only where the whole window lies inside the image: shape (H-10, W-10, C), no padding; the frame's
              SSIM is the mean of the map over positions and channels.  H < 11 or W < 11: ValueError.
  masked      with a mask (N, H, W) bool: psnr_masked takes the MSE over the values of the masked pixels only; ssim_masked is the
              mean of the map over the windows whose CENTRE pixel lies in the mask.  An empty mask gives NaN and a count of 0.
              Without a mask the masked numbers equal the unmasked ones.
  non-finite  (the reference tolerates NaNs in its outputs, loss.py:120) a value that is non-finite in either image is left out of
              the MSE, an SSIM window that contains one is left out of the mean (its map value is NaN); both are counted:
              n_left_out_pixels (values) and n_left_out_windows.
  as_saved    quantises the prediction first the way the reference writes its PNGs (multiply_model.py:1313, astype(np.uint8)
              truncates): floor(clamp(x, 0, 1) * 255) / 255 in float32; the numbers then agree with scoring the saved files.
  mask scores pred, gt (N, P, H, W); gt bool, pred bool or soft opacities cut at `threshold` with >=.  Per person and pooled over
              the persons of a frame: tp = |pred and gt|, n_pred = |pred|, n_gt = |gt|, then iou = tp / (n_pred + n_gt - tp),
              precision = tp / n_pred, recall = tp / n_gt, f1 = 2 tp / (n_pred + n_gt) (= 2 P R / (P + R)).  A zero denominator
              gives 0.
  sequence    the mean of the per-frame values (over the frames where the value is defined, i.e. not NaN), which is how these
              numbers are reported; the per-frame arrays are returned as well.

The SSIM map and the squared errors are device kernels (csrc/image_metrics.hip: window sums, moments and the expression in double
on the float32 inputs -- variances as differences of fp32 raw moments are off by up to 5e-4 per pixel on the mostly flat frames a
renderer produces); the mask counts are plain torch reductions on the device.  This module imports without a device."""
import math

import numpy as np
import torch

from . import hip


def as_images(x, name="image"):
    """(N, H, W, C) float32 HOST-or-device tensor of a tensor / numpy array: (H, W, C) becomes one frame, uint8 is divided by 255.
    TypeError for any other dtype than float32 / uint8, ValueError for any other shape."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[3] not in (1, 3):
        raise ValueError(f"{name}: expected (N, H, W, C) or (H, W, C) with C = 1 or 3, got {tuple(t.shape)}")
    if t.dtype == torch.uint8:
        return _levels(t.device)[t.long()]
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32 or uint8, got {t.dtype}")
    return t


def _levels(device):
    """k / 255, k = 0..255, as float32 divided ON THE HOST: a device division by a constant may be a multiplication by its
    reciprocal, which is one ulp off for some k -- and reading a saved file back gives exactly these"""
    return torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(device)


def quantise_as_saved(x):
    """floor(clamp(x, 0, 1) * 255) / 255 in float32: what reading back the PNG the reference writes gives (NaN stays NaN)"""
    k = torch.floor(torch.clamp(x, 0.0, 1.0) * 255.0)
    return torch.where(torch.isnan(x), x, _levels(x.device)[torch.nan_to_num(k, nan=0.0).long()])


def _checked(pred, gt, mask, need_window):
    pred, gt = as_images(pred, "pred"), as_images(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if need_window and (pred.shape[1] < hip.SSIM_WINDOW or pred.shape[2] < hip.SSIM_WINDOW):
        raise ValueError(f"SSIM needs images of at least {hip.SSIM_WINDOW} x {hip.SSIM_WINDOW} pixels, got "
                         f"{pred.shape[1]} x {pred.shape[2]}")
    if mask is not None:
        mask = mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))
        if mask.dtype != torch.bool:
            raise TypeError(f"mask: expected bool, got {mask.dtype}")
        if mask.dim() == 2:
            mask = mask[None]
        if tuple(mask.shape) != tuple(pred.shape[:3]):
            raise ValueError(f"mask: expected (N, H, W) = {tuple(pred.shape[:3])}, got {tuple(mask.shape)}")
    return pred, gt, mask


def _on_device(pred, gt, mask, as_saved):
    hip.require_device()
    dev = pred.device if pred.is_cuda else (gt.device if gt.is_cuda else torch.device("cuda"))
    pred, gt = pred.to(dev).contiguous(), gt.to(dev).contiguous()
    if as_saved:
        pred = quantise_as_saved(pred)
    return pred, gt, None if mask is None else mask.to(dev).contiguous()


def _ratio(num, den):
    """num / den per frame in float64, NaN where den is 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den > 0)
    return out


def psnr_from_sums(sq_sum, count, data_range=1.0):
    """-10 log10(MSE / data_range^2) per frame from the squared-error sums and counts: +inf for MSE 0, NaN for a count of 0"""
    mse = _ratio(sq_sum, count)
    L = float(np.float32(data_range))
    with np.errstate(divide="ignore"):
        return -10.0 * np.log10(mse / (L * L))


def _mean(values):
    """mean over the frames where the value is defined (not NaN); NaN when there is none"""
    v = np.asarray(values, dtype=np.float64)
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else math.nan


def image_metrics(pred, gt, mask=None, data_range=1.0, as_saved=False, details=None):
    """PSNR and SSIM of the frames pred against gt ((N, H, W, C) or (H, W, C); device or host tensors or numpy arrays; float32 or
    uint8), optionally also inside mask (N, H, W) bool -- the definitions of the module's docstring.  Returns a dict: per-frame
    float64 arrays psnr, ssim, psnr_masked, ssim_masked and their counts n_values, n_windows, n_masked_values, n_masked_windows;
    the sequence means mean_psnr, mean_ssim, mean_psnr_masked, mean_ssim_masked; n_frames, n_left_out_pixels (values) and
    n_left_out_windows.  details: a dict that receives the kernels' sums (N, 5) and the SSIM map (for tests and plots)."""
    pred, gt, mask = _checked(pred, gt, mask, need_window=True)
    pred, gt, mask = _on_device(pred, gt, mask, as_saved)
    sq = hip.image_sqerr(pred, gt, mask)
    ss, smap = hip.image_ssim(pred, gt, mask, data_range, want_map=details is not None)
    if details is not None:
        details.update(sqerr=sq, ssim=ss, ssim_map=smap)
    sq, ss = sq.cpu().numpy(), ss.cpu().numpy()
    out = dict(psnr=psnr_from_sums(sq[:, 0], sq[:, 1], data_range), ssim=_ratio(ss[:, 0], ss[:, 1]),
               psnr_masked=psnr_from_sums(sq[:, 2], sq[:, 3], data_range), ssim_masked=_ratio(ss[:, 2], ss[:, 3]),
               n_values=sq[:, 1].astype(np.int64), n_windows=ss[:, 1].astype(np.int64),
               n_masked_values=sq[:, 3].astype(np.int64), n_masked_windows=ss[:, 3].astype(np.int64))
    for k in ("psnr", "ssim", "psnr_masked", "ssim_masked"):
        out["mean_" + k] = _mean(out[k])
    out.update(n_frames=int(pred.shape[0]), n_left_out_pixels=int(sq[:, 4].sum()), n_left_out_windows=int(ss[:, 4].sum()))
    return out


def psnr(pred, gt, mask=None, data_range=1.0, as_saved=False):
    """per-frame PSNR (N,) float64 of pred against gt, over the masked pixels when a mask (N, H, W) is given (mp_image_sqerr)"""
    pred, gt, mask = _checked(pred, gt, mask, need_window=False)
    pred, gt, mask = _on_device(pred, gt, mask, as_saved)
    sq = hip.image_sqerr(pred, gt, mask).cpu().numpy()
    return psnr_from_sums(sq[:, 2], sq[:, 3], data_range)


def ssim(pred, gt, mask=None, data_range=1.0, as_saved=False, want_map=False):
    """per-frame SSIM (N,) float64 of pred against gt, over the windows centred in the mask when one is given (mp_image_ssim);
    want_map: (ssim, the map (N, H-10, W-10, C) float32 on the device, NaN where a window was left out)"""
    pred, gt, mask = _checked(pred, gt, mask, need_window=True)
    pred, gt, mask = _on_device(pred, gt, mask, as_saved)
    ss, smap = hip.image_ssim(pred, gt, mask, data_range, want_map=want_map)
    ss = ss.cpu().numpy()
    val = _ratio(ss[:, 2], ss[:, 3])
    return (val, smap) if want_map else val


def _zero_safe(num, den):
    return torch.where(den > 0, num.double() / den.double().clamp(min=1), torch.zeros_like(num, dtype=torch.float64))


def mask_scores(tp, n_pred, n_gt):
    """iou, precision, recall, f1 (float64 tensors) from integer count tensors of one shape; a zero denominator gives 0"""
    return dict(iou=_zero_safe(tp, n_pred + n_gt - tp), precision=_zero_safe(tp, n_pred), recall=_zero_safe(tp, n_gt),
                f1=_zero_safe(2 * tp, n_pred + n_gt))


def _as_masks(x, name, threshold=None):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"{name}: expected (N, P, H, W) or (P, H, W), got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        return t
    if threshold is None or not t.dtype.is_floating_point:
        raise TypeError(f"{name}: expected bool" + (" or floating-point opacities" if threshold is not None else "") + f", got {t.dtype}")
    return t >= threshold


def mask_metrics(pred, gt, threshold=0.5):
    """Segmentation scores of the per-person masks pred against gt, both (N, P, H, W) (or (P, H, W): one frame); gt bool, pred bool
    or soft opacities cut with >= threshold.  Returns a dict of float64 / int64 numpy arrays: tp, n_pred, n_gt and iou, precision,
    recall, f1 per frame and person (N, P); the same pooled over the persons of a frame as *_pooled (N,); and the sequence means
    mean_iou, ... per person (P,) and mean_iou_pooled, ... as floats.  The counts are torch reductions on the tensors' device."""
    pred, gt = _as_masks(pred, "pred", threshold), _as_masks(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if torch.cuda.is_available():
        dev = pred.device if pred.is_cuda else (gt.device if gt.is_cuda else torch.device("cuda"))
        pred, gt = pred.to(dev), gt.to(dev)
    counts = dict(tp=(pred & gt).sum((2, 3)), n_pred=pred.sum((2, 3)), n_gt=gt.sum((2, 3)))
    out = {k: v.cpu().numpy() for k, v in counts.items()}
    out.update({k: v.cpu().numpy() for k, v in mask_scores(**counts).items()})
    pooled = {k: v.sum(1) for k, v in counts.items()}
    out.update({k + "_pooled": v.cpu().numpy() for k, v in pooled.items()})
    out.update({k + "_pooled": v.cpu().numpy() for k, v in mask_scores(**pooled).items()})
    for k in ("iou", "precision", "recall", "f1"):
        out["mean_" + k] = out[k].mean(0) if out[k].shape[0] else np.full(out[k].shape[1], np.nan)
        out["mean_" + k + "_pooled"] = float(out[k + "_pooled"].mean()) if out[k].shape[0] else math.nan
    return out


def frame_metrics(outputs, targets, img_size, gt_masks=None, threshold=0.5, **kwargs):
    """Both sets of numbers for ONE eval output dict of Multiply.forward / render_views whose rays are the frame's pixels in
    row-major order: rgb_values (R, 3) against targets (the frame's colours (R, 3) / (H, W, 3), or a dict that holds them as
    "rgb"), R = H W, img_size = (H, W); and, when gt_masks (P, H, W) bool is given, acc_person_list (R, P) cut at `threshold`
    against it.  kwargs go to image_metrics (mask, data_range, as_saved, details).  Returns {"image": ..., "masks": ... or None}."""
    H, W = int(img_size[0]), int(img_size[1])
    rgb = outputs["rgb_values"].detach()
    tgt = targets["rgb"] if isinstance(targets, dict) else targets
    tgt = tgt if torch.is_tensor(tgt) else torch.from_numpy(np.ascontiguousarray(tgt))
    if rgb.numel() != H * W * 3 or tgt.numel() != H * W * 3:
        raise ValueError(f"rgb_values {tuple(rgb.shape)} / targets {tuple(tgt.shape)} do not hold the {H} x {W} pixels of the frame")
    out = {"image": image_metrics(rgb.reshape(1, H, W, 3), tgt.reshape(1, H, W, 3), **kwargs), "masks": None}
    if gt_masks is not None:
        acc = outputs["acc_person_list"].detach()
        if acc.dim() != 2 or acc.shape[0] != H * W:
            raise ValueError(f"acc_person_list {tuple(acc.shape)} does not hold the {H} x {W} pixels of the frame")
        out["masks"] = mask_metrics(acc.reshape(H, W, -1).permute(2, 0, 1)[None], _as_masks(gt_masks, "gt_masks"), threshold)
    return out
