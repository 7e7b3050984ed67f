"""Validation metrics of the shipped option files on the device (csrc/metrics.hip through the C ABI):
psnr / ssim (basicsr.metrics, esrgan_s2naip_urban.yml:153-162) and cpsnr (/root/reference/ssr/metrics/cpsnr.py:8-59); lpips
(/root/reference/ssr/metrics/lpips.py:7-21) is lpips_metric.py and clipscore (ssr/metrics/clipscore.py:9-38) is clipscore_metric.py, both
registered in METRICS below.

Images are uint8 [B, H, W, C] device tensors as `tensor2img_u8` produces them (BasicSR's tensor2img quantisation: clamp to
[0, 1], * 255, round half to even; kept RGB — the three metrics are invariant to the channel order when test_y_channel is false)."""
from __future__ import annotations

import math

import torch

from . import hip


def tensor2img_u8(x: torch.Tensor, truncate: bool = False, check_finite: bool = False, compute_dtype=None) -> torch.Tensor:
    """float32 NCHW on the device -> uint8 NHWC on the device.  truncate=True is the astype(uint8) of infer_grid.py:60-64.
    check_finite=True: count NaN / +-Inf samples in the same pass and raise FloatingPointError (naming `compute_dtype`) if there
    are any, instead of returning the pixels they were clamped to (one read of the counter: a device sync)."""
    if check_finite:
        buf, shape = quantize_u8_checked(x, truncate)
        img, bad = split_checked(buf, shape)
        if bad:
            raise nonfinite_error(bad, compute_dtype)
        return img
    x = x.contiguous().float()
    assert x.is_cuda and x.dim() == 4
    n, c, h, w = x.shape
    out = torch.empty(n, h, w, c, dtype=torch.uint8, device=x.device)
    hip.check(hip.lib().ssr_quantize_u8(x.data_ptr(), out.data_ptr(), n, c, h, w, 1 if truncate else 0, hip.stream_ptr()),
              "ssr_quantize_u8")
    return out


def quantize_u8_checked(x: torch.Tensor, truncate: bool = False):
    """ssr_quantize_u8_checked: -> (one flat uint8 device buffer holding the NHWC image and, at the next 4-byte boundary, the int32
    count of non-finite input samples; the image shape).  One copy of the buffer brings both to the host (split_checked)."""
    x = x.contiguous().float()
    assert x.is_cuda and x.dim() == 4
    n, c, h, w = x.shape
    off = -(-n * h * w * c // 4) * 4
    buf = torch.empty(off + 4, dtype=torch.uint8, device=x.device)
    cnt = buf[off:].view(torch.int32)
    cnt.zero_()
    hip.check(hip.lib().ssr_quantize_u8_checked(x.data_ptr(), buf.data_ptr(), n, c, h, w, 1 if truncate else 0, cnt.data_ptr(),
                                                 hip.stream_ptr()), "ssr_quantize_u8_checked")
    return buf, (n, h, w, c)


def split_checked(buf: torch.Tensor, shape):
    """a buffer of quantize_u8_checked (on the device or copied to the host) -> (uint8 image view [N, H, W, C], non-finite count)"""
    nb = math.prod(shape)
    off = -(-nb // 4) * 4
    return buf[:nb].view(shape), int(buf[off:off + 4].view(torch.int32)[0])


def nonfinite_error(count: int, compute_dtype=None, where: str = "") -> FloatingPointError:
    """what inference / validation raise instead of writing pixels derived from NaN / Inf"""
    msg = f"{count} non-finite output sample(s){where}" + (f" in compute_dtype {compute_dtype}" if compute_dtype is not None else "")
    if compute_dtype == "fp32h":
        msg += (": fp32h runs the forward convolutions on fp16-split operands (|activation| < 65504, |weight| < 64); "
                "set `compute_dtype: fp32f` (exact fp32 forward, same gates) for this model")
    return FloatingPointError(msg)


def _pair(a, b):
    assert a.shape == b.shape and a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.is_cuda and b.is_cuda, \
        f"Image shapes are different: {tuple(a.shape)}, {tuple(b.shape)}."
    if a.dim() == 4:
        assert a.shape[0] == 1, "one image per call (the reference validates with batch size 1)"
        a, b = a[0], b[0]
    return a.contiguous(), b.contiguous()


def _no_y(test_y_channel):
    if test_y_channel:
        raise NotImplementedError("metrics with test_y_channel: true (no shipped option file uses it)")


def _shift_sums(a, b, crop, m):
    h, w, c = a.shape
    out = torch.empty((m + 1) ** 2, c, 2, dtype=torch.int64, device=a.device)
    hip.check(hip.lib().ssr_metric_shift_sums(a.data_ptr(), b.data_ptr(), h, w, c, crop, m, out.data_ptr(), hip.stream_ptr()),
              "ssr_metric_shift_sums")
    return out.cpu(), (h - 2 * crop - m) * (w - 2 * crop - m)


def calculate_psnr(img, img2, crop_border, input_order="HWC", test_y_channel=False, **kw) -> float:
    _no_y(test_y_channel)
    a, b = _pair(img, img2)
    s, n = _shift_sums(a, b, crop_border, 0)
    mse = int(s[0, :, 1].sum()) / (n * a.shape[2])
    return float("inf") if mse == 0 else 10.0 * math.log10(255.0 * 255.0 / mse)


def calculate_cpsnr(img, img2, crop_border, input_order="HWC", test_y_channel=False, **kw) -> float:
    """cpsnr.py:36-55: for each of the 81 relative offsets the per-channel mean difference is removed before the MSE:
    mean((d - mean d)^2) = (S2 - S1^2 / n) / n per channel, averaged over the channels."""
    _no_y(test_y_channel)
    a, b = _pair(img, img2)
    s, n = _shift_sums(a, b, crop_border, 8)
    s = s.double()
    mse = ((s[:, :, 1] - s[:, :, 0] ** 2 / n) / n).mean(dim=1)
    best = float(mse.min())
    return float("inf") if best == 0 else 10.0 * math.log10(255.0 * 255.0 / best)


def calculate_ssim(img, img2, crop_border, input_order="HWC", test_y_channel=False, **kw) -> float:
    _no_y(test_y_channel)
    a, b = _pair(img, img2)
    h, w, c = a.shape
    out = torch.empty(c, dtype=torch.float64, device=a.device)
    hip.check(hip.lib().ssr_metric_ssim_sums(a.data_ptr(), b.data_ptr(), h, w, c, crop_border, out.data_ptr(), hip.stream_ptr()),
              "ssr_metric_ssim_sums")
    n = (h - 2 * crop_border - 10) * (w - 2 * crop_border - 10)
    return float((out.cpu() / n).mean())


from .lpips_metric import calculate_lpips, check_lpips_opt  # noqa: E402  (ssr/metrics/lpips.py: VGG16 forward + csrc/lpips.hip)
from .clipscore_metric import calculate_clipscore, check_clipscore_opt  # noqa: E402  (ssr/metrics/clipscore.py: ViT forward, csrc/vit.hip)

METRICS = {"calculate_psnr": calculate_psnr, "calculate_ssim": calculate_ssim, "calculate_cpsnr": calculate_cpsnr,
           "calculate_lpips": calculate_lpips, "calculate_clipscore": calculate_clipscore}
# what a metric needs checked BEFORE the first image is processed (called with the entry's keys, without `type` / `better`):
# calculate_lpips and calculate_clipscore validate their keys and find their weights files
METRIC_CHECKS = {"calculate_lpips": check_lpips_opt, "calculate_clipscore": check_clipscore_opt}


def imwrite_rgb(img_hwc_u8, path: str):
    """basicsr imwrite (cv2.imwrite of a BGR array) writes the same PNG pixels as saving the RGB array directly."""
    from PIL import Image
    Image.fromarray(img_hwc_u8).save(path)
