"""Shared by the CLIP-loss tests and tools/make_cliploss_golden.py: the two rule-filled tiny SigLIP towers, the fixture images and the
loader of tests/golden/cliploss_siglip_tiny.pt.  (Not a test module.)  No weights are committed: the towers are filled by the rule of
tests/clipscore_fixture.py.

    A   width 128, 2 heads of 64, MLP 200, depth 2, patch 16, grid 9: 81 tokens (crosses the 64-key tile), image_size 144
    B   clipscore_fixture.TINY["siglip"]: width 144, 2 heads of 72, MLP 200, depth 2, patch 14, grid 3: 9 tokens, image_size 42
    images: B = 3 at 36 x 36 (an integer ratio to 144) and 50 x 40 (non-integer ratios), float32 values k / 255 (stored as uint8 k)
"""
import os

import torch

import clipscore_fixture as FX

TOWERS = {"A": dict(width=128, heads=2, mlp=200, depth=2, patch=16, grid=9), "B": dict(FX.TINY["siglip"])}
TOWER_SEED = {"A": 5, "B": FX.SEED["siglip"]}
SIZES = ((36, 36), (50, 40))
LOSS_WEIGHT = 0.75                                  # not 1: a dropped weight shows
SIGN_MARGIN = 1e-3                                  # min|fx - fg| >= SIGN_MARGIN * max|fx| in float64: no sign flips under fp32 rounding
PATH = os.path.join(FX.GOLDEN, "cliploss_siglip_tiny.pt")


def tower_state(name: str):
    return FX.rule_state("siglip", TOWER_SEED[name], **TOWERS[name])


def images(seed: int, h: int, w: int):
    """-> fake, gt: uint8 [3, 3, h, w] (to_float: float32 k / 255); gt is a smooth pattern plus noise, fake an even mix of it with fresh noise in
    two images and unrelated noise in the third"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) / h, torch.arange(w, dtype=torch.float32) / w, indexing="ij")
    base = torch.stack([yy, xx, 1 - 0.5 * (yy + xx)])
    gt = (0.6 * base[None] + 0.4 * torch.rand(3, 3, h, w, generator=g)).clamp(0, 1)
    fake = (0.5 * gt + 0.5 * torch.rand(3, 3, h, w, generator=g)).clamp(0, 1)
    fake[2] = torch.rand(3, h, w, generator=g)
    return (fake * 255).round().to(torch.uint8).contiguous(), (gt * 255).round().to(torch.uint8).contiguous()


def to_float(u8: torch.Tensor) -> torch.Tensor:
    """float32 k / 255 (IEEE division)"""
    return u8.to(torch.float32) / 255


def load_golden():
    return torch.load(PATH, weights_only=False)


def case_key(tower: str, h: int, w: int) -> str:
    return f"{tower}:{h}x{w}"
