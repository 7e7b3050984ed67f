"""L2Model's networks and loss stated in plain torch for the CPU, and NumPy statements of the kernels of csrc/l2net.hip: what the
device is tested against, and what runs without a GPU.  Written from the behaviour of the WorldStrat baselines the reference ships
(ssr/archs/srcnn_arch.py, highresnet_arch.py, arch_util.py:65-598; ssr/models/ssr_l2_model.py:30-52), not from their text.

    srcnn_reference(sd, x, masks=None)        SRCNN forward from a state_dict; differentiable, any float dtype
    highresnet_reference(sd, x, masks=None)   HighResNet forward
    l2_loss_reference(out, gt)                {'mse', 'mae', 'ssim', 'tot_loss', 'psnr_loss'} of L2Model's hard-coded loss
    philox_keep_bits / pack_mask_nhwc / prelu_reflect_fwd_np / prelu_reflect_bwd_np / sr_tail_reference
                                               the kernels, restated

`x` is [B, revisits, C, H, W]; the result is [B, 1, out_channels, zoom H, zoom W].  `masks` is None (eval: Dropout is the identity)
or a list of bool keep-masks, one per dropout site in forward order, each shaped like the activation it multiplies (NCHW); a kept
element is scaled by 2 (p = 0.5).  The networks' sizes are read off the state_dict's shapes.

A 3 x 3 convolution here is padding='same' with padding_mode='reflect': one pixel of reflect padding that does not repeat the edge.
"""
from __future__ import annotations

import math
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from .ssim_loss import ssim_loss_reference

W_MSE, W_MAE, W_SSIM = 0.3, 0.4, 0.3       # ssr_l2_model.py:36-40 (the WorldStrat paper's weights)


def _conv_reflect(x, w, b):
    p = w.shape[-1] // 2
    if p:
        x = F.pad(x, (p, p, p, p), mode="reflect")
    return F.conv2d(x, w, b)


def _prelu(x, a):
    return torch.where(x > 0, x, a * x)


def _drop(x, masks: Optional[Iterator]):
    if masks is None:
        return x
    m = next(masks)
    assert m.shape == x.shape, f"dropout mask {tuple(m.shape)} for an activation {tuple(x.shape)}"
    return x * m.to(x.dtype) * 2


def _double_conv(sd, p, x, masks):
    """conv, PReLU, Dropout, conv, PReLU, Dropout (keys p + '0.weight' .. '6.weight')"""
    x = _drop(_prelu(_conv_reflect(x, sd[p + "0.weight"], sd[p + "0.bias"]), sd[p + "2.weight"]), masks)
    return _drop(_prelu(_conv_reflect(x, sd[p + "4.weight"], sd[p + "4.bias"]), sd[p + "6.weight"]), masks)


def _sr(sd, x, zoom):
    x = F.pixel_shuffle(x, zoom)
    x = _prelu(_conv_reflect(x, sd["sr.upsample.1.weight"], sd["sr.upsample.1.bias"]), sd["sr.upsample.3.weight"])
    return _prelu(_conv_reflect(x, sd["sr.upsample.4.weight"], sd["sr.upsample.4.bias"]), sd["sr.upsample.6.weight"])


def zoom_of(sd) -> int:
    hidden = sd["encoder.doubleconv2d.4.weight"].shape[0]
    return int(round(math.sqrt(hidden // sd["sr.upsample.1.weight"].shape[0])))


def _count(sd, fmt: str) -> int:
    n = 0
    while fmt.format(n) in sd:
        n += 1
    return n


def _cast(sd, dtype):
    return {k: (v if v.dtype == dtype else v.to(dtype)) for k, v in sd.items()}


def srcnn_reference(sd: Dict[str, torch.Tensor], x: torch.Tensor, masks: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    sd = _cast(sd, x.dtype)
    it = iter(masks) if masks is not None else None
    B, R, C, H, W = x.shape
    hidden = sd["encoder.doubleconv2d.4.weight"].shape[0]
    h = _double_conv(sd, "encoder.doubleconv2d.", x.reshape(B * R, C, H, W), it)
    h = h.reshape(B, R * hidden, H, W)                      # revisits become channels
    h = _double_conv(sd, "doubleconv2d.doubleconv2d.", h, it)
    for i in range(_count(sd, "residualblocks.{}.residualblock.doubleconv2d.0.weight")):
        h = h + _double_conv(sd, f"residualblocks.{i}.residualblock.doubleconv2d.", h, it)
    return _sr(sd, h, zoom_of(sd))[:, None]


def highresnet_reference(sd: Dict[str, torch.Tensor], x: torch.Tensor, masks: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    sd = _cast(sd, x.dtype)
    it = iter(masks) if masks is not None else None
    B, R, C, H, W = x.shape
    hidden = sd["encoder.doubleconv2d.4.weight"].shape[0]
    h = _double_conv(sd, "encoder.doubleconv2d.", x.reshape(B * R, C, H, W), it).reshape(B, R, hidden, H, W)
    levels = _count(sd, "fusion.fusion.{}.fuse.1.weight")
    if R < 2 ** levels:                                      # zero revisits behind the encoded ones, up to a power of two
        h = torch.cat([h, h.new_zeros(B, 2 ** levels - R, hidden, H, W)], dim=1)
    for i in range(levels):
        half = h.shape[1] // 2
        p = f"fusion.fusion.{i}.fuse."
        z = torch.cat([h[:, :half].reshape(B * half, hidden, H, W), h[:, half:].reshape(B * half, hidden, H, W)], dim=1)
        z = z + _double_conv(sd, p + "0.residualblock.doubleconv2d.", z, it)
        z = _prelu(_conv_reflect(z, sd[p + "1.weight"], sd[p + "1.bias"]), sd[p + "3.weight"])
        h = z.reshape(B, half, hidden, H, W)
    return _sr(sd, h[:, 0], zoom_of(sd))[:, None]


def l2_loss_reference(out: torch.Tensor, gt: torch.Tensor) -> Dict[str, torch.Tensor]:
    """out, gt: [B, C, H, W].  The reference averages per-sample means over the batch; with equal sample sizes that is the plain mean."""
    d = out - gt
    mse, mae = (d * d).mean(), d.abs().mean()
    ssim = ssim_loss_reference(out, gt)
    return {"psnr_loss": 10.0 * torch.log10(mse), "mse": mse, "mae": mae, "ssim": ssim,
            "tot_loss": W_MSE * mse + W_MAE * mae + W_SSIM * ssim}


def dropout_site_shapes(arch: str, B: int, R: int, H: int, W: int, hidden: int, residual_layers: int) -> List[tuple]:
    """NCHW shapes of the dropout sites in forward order"""
    s = [(B * R, hidden, H, W)] * 2
    if arch == "SRCNN":
        return s + [(B, hidden, H, W)] * (2 + 2 * residual_layers)
    n = 1 << max(0, (R - 1).bit_length())
    while n > 1:
        n //= 2
        s += [(B * n, 2 * hidden, H, W)] * 2
    return s


# ------------------------------------------------------------------------------------------------ the kernels, restated
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox_keep_bits(seed: int, step: int, layer: int, n_words: int) -> np.ndarray:
    """ssr_dropout_mask: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (j & 0xffffffff, j >> 32, step, layer) -> words
    4j .. 4j+3.  Returns uint32 [n_words] (n_words % 4 == 0)."""
    assert n_words % 4 == 0
    j = np.arange(n_words // 4, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = j & m32, j >> np.uint64(32)
    c2 = np.full_like(j, np.uint64(step & 0xFFFFFFFF))
    c3 = np.full_like(j, np.uint64(layer & 0xFFFFFFFF))
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32).reshape(-1)


def mask_words(n_elems: int) -> int:
    """words of a packed mask over n_elems elements, rounded up to whole Philox blocks of 128 bits"""
    return (n_elems + 127) // 128 * 4


def unpack_bits(words: np.ndarray, n_elems: int) -> np.ndarray:
    """bool [n_elems]: bit (e & 31) of word (e >> 5)"""
    e = np.arange(n_elems, dtype=np.int64)
    return ((words[e >> 5] >> (e & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def pack_mask_nhwc(mask_nchw: torch.Tensor) -> np.ndarray:
    """a bool NCHW keep-mask as the packed words the kernels read (element order N, H, W, C)"""
    flat = mask_nchw.permute(0, 2, 3, 1).reshape(-1).cpu().numpy().astype(bool)
    n = flat.size
    padded = np.zeros(mask_words(n) * 32, dtype=bool)
    padded[:n] = flat
    return np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32).copy()


def _reflect(i: int, n: int) -> int:
    return -i if i < 0 else (2 * n - 2 - i if i >= n else i)


def prelu_reflect_fwd_np(pre, a, keep=None, res=None, pad=1):
    """ssr_prelu_reflect_fwd on NHWC float32 arrays: pre [N, H, W, C], keep bool like pre or None, res [N, H, W, C] or None.
    Every step is one float32 operation, as in the kernel.  Returns [N, H + 2 pad, W + 2 pad, C]."""
    f = np.float32
    pre = pre.astype(f)
    v = np.where(pre > 0, pre, f(a) * pre).astype(f)
    if keep is not None:
        v = np.where(keep, v * f(2), f(0)).astype(f)
    if res is not None:
        v = (res.astype(f) + v).astype(f)
    if not pad:
        return v
    N, H, W, C = v.shape
    yi = [_reflect(p - 1, H) for p in range(H + 2)]
    xi = [_reflect(p - 1, W) for p in range(W + 2)]
    return v[:, yi][:, :, xi]


def fold_np(g, H, W, pad, acc=None):
    """the kernel's running float32 sum of the padded-grid samples that read interior (y, x): rows, then columns, in increasing
    padded index, continued from `acc` when given"""
    f = np.float32
    if not pad:
        return g.astype(f) if acc is None else (acc + g.astype(f)).astype(f)
    out = None if acc is None else acc.copy()
    N, C = g.shape[0], g.shape[-1]
    res = np.zeros((N, H, W, C), dtype=f)
    for y in range(H):
        rows = ([0] if y == 1 else []) + [y + 1] + ([H + 1] if y == H - 2 else [])
        for x in range(W):
            cols = ([0] if x == 1 else []) + [x + 1] + ([W + 1] if x == W - 2 else [])
            s = None if out is None else out[:, y, x]
            for r in rows:
                for c in cols:
                    s = g[:, r, c].astype(f) if s is None else (s + g[:, r, c].astype(f)).astype(f)
            res[:, y, x] = s
    return res


def prelu_reflect_bwd_np(pre, a, g, g_pad=1, keep=None, g2=None, g2_pad=1):
    """ssr_prelu_reflect_bwd: returns (dpre float32, the terms of d loss / d slope as float64 [N, H, W, C])"""
    f = np.float32
    N, H, W, C = pre.shape
    t = fold_np(g, H, W, g_pad)
    if g2 is not None:
        t = fold_np(g2, H, W, g2_pad, acc=t)
    if keep is not None:
        t = np.where(keep, t * f(2), f(0)).astype(f)
    pos = pre > 0
    dpre = np.where(pos, t, f(a) * t).astype(f)
    terms = np.where(pos, 0.0, pre.astype(np.float64) * t.astype(np.float64))
    return dpre, terms


def sr_tail_reference(x_nhwc: torch.Tensor, w1, b1, s1, w2, b2, s2, zoom: int) -> torch.Tensor:
    """ssr_sr_tail_fwd in torch (differentiable, any dtype): x [N, H, W, hidden] -> [N, zoom H, zoom W, Cout]"""
    x = F.pixel_shuffle(x_nhwc.permute(0, 3, 1, 2), zoom)
    cm, co = w1.shape[0], w2.shape[0]
    x = _prelu(F.conv2d(x, w1.reshape(cm, cm, 1, 1), b1), s1)
    x = _prelu(F.conv2d(x, w2.reshape(co, cm, 1, 1), b2), s2)
    return x.permute(0, 2, 3, 1)
