"""BasicSR's pixel and GAN losses stated in torch for the CPU: what ssr_l1_loss / ssr_pixel_loss and ssr_bce_logits_loss /
ssr_gan_loss (csrc/misc.hip, csrc/losses.hip) compute on the device.

BasicSR 1.4.2, which `SSRESRGANModel` builds its criteria from with `build_loss`:

    basicsr/losses/basic_loss.py   L1Loss, MSELoss, CharbonnierLoss: loss_weight * mean(|d|), mean(d^2), mean(sqrt(d^2 + eps)), d = pred - target
    basicsr/losses/gan_loss.py     GANLoss.forward(input, target_is_real, is_disc): vanilla (BCEWithLogitsLoss) and lsgan (MSELoss) against a
                                   constant label map; wgan, wgan_softplus and hinge ignore the label values (get_target_label);
                                   loss_weight applies to the generator's term only (is_disc=False)

    pixel_loss_reference / gan_loss_reference            the loss, differentiable, any float dtype
    pixel_loss_grad_reference / gan_loss_grad_reference  (loss, d loss / d pred) in closed form
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn.functional as F

PIXEL_TYPES = ("L1Loss", "MSELoss", "CharbonnierLoss")
GAN_TYPES = ("vanilla", "lsgan", "wgan", "wgan_softplus", "hinge")
CHARBONNIER_EPS = 1e-12          # CharbonnierLoss.__init__'s default


def softplus(z: torch.Tensor) -> torch.Tensor:
    """log(1 + exp(z)) = max(z, 0) + log1p(exp(-|z|)), which is how logaddexp evaluates it: finite for every finite z, and with
    sigmoid(z) as its autograd derivative at z == 0 too (the max / |z| form written out has a kink there).  F.softplus switches to z
    beyond its threshold of 20, where the two differ by log1p(exp(-20)) < 3e-9"""
    return torch.logaddexp(z, torch.zeros_like(z))


def pixel_loss_reference(pred: torch.Tensor, target: torch.Tensor, kind: str = "L1Loss", weight: float = 1.0,
                         eps: float = CHARBONNIER_EPS) -> torch.Tensor:
    d = pred - target
    if kind == "L1Loss":
        return weight * d.abs().mean()
    if kind == "MSELoss":
        return weight * (d * d).mean()
    if kind == "CharbonnierLoss":
        return weight * torch.sqrt(d * d + eps).mean()
    raise NotImplementedError(f"pixel loss {kind!r}: one of {PIXEL_TYPES}")


def pixel_loss_grad_reference(pred: torch.Tensor, target: torch.Tensor, kind: str = "L1Loss", weight: float = 1.0,
                              eps: float = CHARBONNIER_EPS) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, d loss / d pred):  w sign(d) / n,  2 w d / n,  w d / (n sqrt(d^2 + eps)) - 0 where d == 0 in all three"""
    with torch.no_grad():
        d = pred - target
        k = weight / d.numel()
        if kind == "L1Loss":
            grad = k * torch.sign(d)
        elif kind == "MSELoss":
            grad = 2 * k * d
        elif kind == "CharbonnierLoss":
            grad = torch.where(d == 0, torch.zeros_like(d), k * d / torch.sqrt(d * d + eps))
        else:
            raise NotImplementedError(f"pixel loss {kind!r}: one of {PIXEL_TYPES}")
        return pixel_loss_reference(pred, target, kind, weight, eps), grad


def gan_loss_reference(pred: torch.Tensor, gan_type: str, target_is_real: bool, is_disc: bool, loss_weight: float = 1.0,
                       real_label_val: float = 1.0, fake_label_val: float = 0.0) -> torch.Tensor:
    """GANLoss(gan_type, real_label_val, fake_label_val, loss_weight).forward(pred, target_is_real, is_disc)"""
    t = real_label_val if target_is_real else fake_label_val
    if gan_type == "vanilla":       # BCEWithLogits against t: softplus(x) - x t
        loss = (softplus(pred) - pred * t).mean()
    elif gan_type == "lsgan":
        loss = ((pred - t) ** 2).mean()
    elif gan_type == "wgan":
        loss = -pred.mean() if target_is_real else pred.mean()
    elif gan_type == "wgan_softplus":
        loss = softplus(-pred).mean() if target_is_real else softplus(pred).mean()
    elif gan_type == "hinge":
        if is_disc:
            loss = F.relu(1 + (-pred if target_is_real else pred)).mean()
        else:                       # the generator's term does not look at target_is_real
            loss = -pred.mean()
    else:
        raise NotImplementedError(f"gan_type {gan_type!r}: one of {GAN_TYPES}")
    return loss if is_disc else loss * loss_weight


def gan_loss_grad_reference(pred: torch.Tensor, gan_type: str, target_is_real: bool, is_disc: bool, loss_weight: float = 1.0,
                            real_label_val: float = 1.0, fake_label_val: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(loss, d loss / d pred) with w = 1 for is_disc, loss_weight otherwise, and n = pred.numel():
        vanilla        w (sigmoid(x) - t) / n
        lsgan          2 w (x - t) / n
        wgan           real -w / n, fake w / n
        wgan_softplus  real w (sigmoid(x) - 1) / n, fake w sigmoid(x) / n
        hinge          is_disc: real -[1 - x > 0] / n, fake [1 + x > 0] / n (relu'(0) = 0, as torch); generator -w / n"""
    with torch.no_grad():
        x = pred
        t = real_label_val if target_is_real else fake_label_val
        k = (1.0 if is_disc else loss_weight) / x.numel()
        sgn = -1.0 if target_is_real else 1.0
        if gan_type == "vanilla":
            grad = k * (torch.sigmoid(x) - t)
        elif gan_type == "lsgan":
            grad = 2 * k * (x - t)
        elif gan_type == "wgan":
            grad = torch.full_like(x, sgn * k)
        elif gan_type == "wgan_softplus":
            grad = sgn * k * torch.sigmoid(sgn * x)        # -sigmoid(-x) = sigmoid(x) - 1 without the cancellation
        elif gan_type == "hinge":
            if is_disc:
                grad = torch.where(1 + sgn * x > 0, torch.full_like(x, sgn * k), torch.zeros_like(x))
            else:
                grad = torch.full_like(x, -k)
        else:
            raise NotImplementedError(f"gan_type {gan_type!r}: one of {GAN_TYPES}")
        return gan_loss_reference(pred, gan_type, target_is_real, is_disc, loss_weight, real_label_val, fake_label_val), grad
