"""The SSIM loss of `train.ssim_opt` (type SSIMLoss) stated in torch for the CPU: what csrc/ssim.hip computes on the device.

The reference (ssr/losses/basic_loss.py:50-60, called at ssr_esrgan_model.py:163-166) is
`loss_weight * kornia.losses.ssim_loss(output, percep_gt, window_size=5, reduction="none").mean()`.  kornia is not a dependency
of this package and the reference pins no version, so the definition here is kornia's documented `ssim_loss` / `metrics.ssim`
with their defaults (max_val = 1.0, eps = 1e-12, padding = "same"): a 5 x 5 Gaussian window (sigma 1.5), 2-pixel reflect padding
without repeating the edge, C1 = 0.01^2, C2 = 0.03^2.  It was written from that documentation and could not be executed against
kornia itself ("SSIM loss").

    ssim_loss_reference       the loss, differentiable, any float dtype, NCHW
    ssim_loss_grad_reference  (loss, d loss / d x) in closed form, with the transpose of the reflect-padded filter
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

WINDOW_SIZE = 5
SIGMA = 1.5
C1 = 0.01 ** 2
C2 = 0.03 ** 2
EPS = 1e-12


def window(dtype=torch.float64) -> torch.Tensor:
    """g[i] = exp(-(i - 2)^2 / (2 * 1.5^2)) / sum: 0.12008, 0.23388, 0.29208, 0.23388, 0.12008"""
    i = torch.arange(WINDOW_SIZE, dtype=torch.float64) - WINDOW_SIZE // 2
    g = torch.exp(-i * i / (2 * SIGMA * SIGMA))
    return (g / g.sum()).to(dtype)


def _filter(z: torch.Tensor) -> torch.Tensor:
    """F(z): the separable 5 x 5 Gaussian over 2-pixel reflect padding, per plane of an NCHW tensor"""
    c = z.shape[1]
    g = window(z.dtype).to(z.device)
    k = torch.outer(g, g).expand(c, 1, WINDOW_SIZE, WINDOW_SIZE)
    return F.conv2d(F.pad(z, (2, 2, 2, 2), mode="reflect"), k, groups=c)


def _terms(x, y):
    mx, my = _filter(x), _filter(y)
    exx, eyy, exy = _filter(x * x), _filter(y * y), _filter(x * y)
    a1 = 2 * mx * my + C1
    a2 = 2 * (exy - mx * my) + C2
    b1 = mx * mx + my * my + C1
    b2 = (exx - mx * mx) + (eyy - my * my) + C2
    d = b1 * b2 + EPS
    return mx, my, a1, a2, b1, b2, d, a1 * a2 / d


def ssim_map(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """S of every pixel and channel plane (NCHW, H and W >= 3)"""
    return _terms(x, y)[-1]


def ssim_loss_reference(x: torch.Tensor, y: torch.Tensor, loss_weight: float = 1.0) -> torch.Tensor:
    """loss_weight * mean(clamp((1 - S) / 2, 0, 1)) over all B*C*H*W elements (= the reference's mean of per-image means)"""
    assert x.shape == y.shape and x.dim() == 4 and min(x.shape[-2:]) >= 3, "NCHW, H and W >= 3 (2-pixel reflect padding)"
    return loss_weight * torch.clamp((1 - ssim_map(x, y)) / 2, 0, 1).mean()


def fold_matrix(n: int, dtype=torch.float64) -> torch.Tensor:
    """M[p, q] = sum of g[t + 2] over t in -2 .. 2 with reflect(p + t) == q: one axis of F as a matrix, F(z) = M z.  Its transpose
    is Ft: rows 1, 2, n-3 and n-2 of Ft's output receive the taps folded in from the padding, rows 0 and n-1 none (at n = 3, where
    n-3 = 0 and 2 = n-1, they are among the four); at n = 3 and n = 4 one row receives folds from both ends."""
    assert n >= 3
    g = window(torch.float64)
    m = torch.zeros(n, n, dtype=torch.float64)
    for p in range(n):
        for t in range(-2, 3):
            q = p + t
            q = -q if q < 0 else (2 * (n - 1) - q if q >= n else q)
            m[p, q] += g[t + 2]
    return m.to(dtype)


def ssim_loss_grad_reference(x: torch.Tensor, y: torch.Tensor, loss_weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, d loss / d x) without autograd:  d l / d x = Ft(a) + 2 x Ft(b) + y Ft(c)  with
        k = -loss_weight / (2 * numel) where 0 <= (1 - S) / 2 <= 1, else 0          (torch's clamp gradient)
        a = k (2 my (A2 - A1) / D - 2 mx S (B2 - B1) / D),   b = k (-S B1 / D),   c = k (2 A1 / D)
    and Ft the transpose of F: per axis the transpose of fold_matrix (NOT reflect-padded filtering)."""
    assert x.shape == y.shape and x.dim() == 4 and min(x.shape[-2:]) >= 3
    with torch.no_grad():
        mx, my, a1, a2, b1, b2, d, s = _terms(x, y)
        v = (1 - s) / 2
        k = torch.where((v >= 0) & (v <= 1), torch.full_like(v, -loss_weight / (2 * x.numel())), torch.zeros_like(v))
        a = k * (2 * my * (a2 - a1) / d - 2 * mx * s * (b2 - b1) / d)
        b = k * (-s * b1 / d)
        c = k * (2 * a1 / d)
        mh, mw = fold_matrix(x.shape[-2], x.dtype).to(x.device), fold_matrix(x.shape[-1], x.dtype).to(x.device)
        ft = lambda z: mh.t() @ z @ mw             # noqa: E731  rows: Mh^T z, columns: (Mw^T z^T)^T = z Mw
        grad = ft(a) + 2 * x * ft(b) + y * ft(c)
        loss = loss_weight * torch.clamp(v, 0, 1).mean()
    return loss, grad
