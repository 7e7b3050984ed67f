"""`tower_arithmetic: split` of train.clip_opt and of calculate_clipscore: the tower's matrix products on split operands
(csrc/linear_split.hip, ssr_linear_split in include/ssr_hip.h).

Every fp32 operand v is two 16-bit pieces, hi = round16(v) and lo = round16(v - hi); a product keeps x_hi w_hi + x_hi w_lo + x_lo w_hi.

    pieces "f16"   the forward: fp16 pieces, W multiplied by 2^10 before its split, the sum by 2^-10 after.  |x| < 65504, |w| < 64
    pieces "bf16"  the data gradient dX = dY W: bf16 pieces, no scale (gradients of 1e-8 .. 1e-4 lie below fp16's range)

    linear_split_reference     the arithmetic model the kernel is held to: the three piece products in float64
    split_representation_bound what the model may differ from the exact product by, per output
    check_tower_arithmetic     the option's values
    check_tower_attention      the values of the sibling option `tower_attention: fma | mfma` (csrc/mha_mfma.hip), check_mfma_head_dim
    check_split_domain         |w| < 64 for every matrix, by name, on the host
    pack_split_weight          ssr_linear_split_pack into a fresh device buffer
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

TOWER_ARITHMETICS = ("exact", "split")
SPLIT_WSCALE = 1024.0                   # 2^SSR_F32H_WSHIFT
SPLIT_W_LIMIT = 64.0                    # 2^10 * 64 = 65536 > 65504: the hi piece of a scaled weight would be infinite
_DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}


def check_tower_arithmetic(value, where: str) -> str:
    """`where` names the option in the refusal, e.g. 'train.clip_opt.tower_arithmetic'; None (an absent key) is 'exact'"""
    value = "exact" if value is None else value
    if value not in TOWER_ARITHMETICS:
        raise NotImplementedError(f"{where}={value!r} (have {list(TOWER_ARITHMETICS)})")
    return value


TOWER_ATTENTIONS = ("fma", "mfma")      # ssr_mha_fwd / ssr_mha_bwd | ssr_mha_mfma_fwd / ssr_mha_mfma_bwd (csrc/mha_mfma.hip)
MFMA_HEAD_DIMS = (64, 72)               # the head dims ssr_mha_mfma_* take


def check_tower_attention(value, where: str) -> str:
    """`tower_attention` of train.clip_opt and of calculate_clipscore: which kernels run the blocks' self-attention, 'fma' (the
    default, and what None, an absent key, means) or 'mfma' (the fp32-input matrix core; same mathematics, another order of
    additions).  Orthogonal to tower_arithmetic.  `where` names the option in the refusal."""
    value = "fma" if value is None else value
    if value not in TOWER_ATTENTIONS:
        raise NotImplementedError(f"{where}={value!r} (have {list(TOWER_ATTENTIONS)})")
    return value


def check_mfma_head_dim(head_dim: int, where: str) -> None:
    """a tower whose head dim ssr_mha_mfma_* do not take is refused by name, on the host, when the plan is built"""
    if head_dim not in MFMA_HEAD_DIMS:
        raise NotImplementedError(f"{where}: tower_attention 'mfma' takes head dims {list(MFMA_HEAD_DIMS)}, this tower has {head_dim}; use "
                                  "tower_attention 'fma'")


def split_pieces(t: torch.Tensor, pieces: str):
    """fp32 values (anything else is rounded to fp32 first, as a device buffer holds it) -> (hi, lo) in float64"""
    dt = _DTYPES[pieces]
    t32 = t.to(torch.float32)
    hi = t32.to(dt)
    lo = (t32 - hi.to(torch.float32)).to(dt)
    return hi.to(torch.float64), lo.to(torch.float64)


def linear_split_reference(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], pieces: str) -> torch.Tensor:
    """x [..., K], w [Nout, K], bias [Nout] or None -> float64 [..., Nout]: x_hi w_hi + x_hi w_lo + x_lo w_hi (+ bias) with the pieces
    formed by torch's .half() / .bfloat16() and, for 'f16', the weight scaled by 2^10 before the split and the sum by 2^-10 after."""
    f16 = pieces == "f16"
    xh, xl = split_pieces(x, pieces)
    wh, wl = split_pieces(w.to(torch.float32) * SPLIT_WSCALE if f16 else w, pieces)
    y = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    if f16:
        y = y / SPLIT_WSCALE
    if bias is not None:
        y = y + bias.to(torch.float64)
    return y


def split_piece_magnitude(x: torch.Tensor, w: torch.Tensor, pieces: str) -> torch.Tensor:
    """sum_k of |x_hi w_hi| + |x_hi w_lo| + |x_lo w_hi| (unscaled for 'f16'): what a summation-order bound multiplies"""
    f16 = pieces == "f16"
    xh, xl = (p.abs() for p in split_pieces(x, pieces))
    wh, wl = (p.abs() for p in split_pieces(w.to(torch.float32) * SPLIT_WSCALE if f16 else w, pieces))
    m = xh @ wh.t() + xh @ wl.t() + xl @ wh.t()
    return m / SPLIT_WSCALE if f16 else m


def split_representation_bound(x: torch.Tensor, w: torch.Tensor, pieces: str) -> torch.Tensor:
    """|linear_split_reference - the exact product| per output, at most:
      f16   2^-20 mag + 2^-25 sum_k |w_k| + 2^-35 sum_k |x_k|      mag = sum_k |x_k w_k|
            (2^-22 each for the residual x - hi - lo, the residual of w and the dropped x_lo w_lo: a piece keeps 11 bits;  the
            other two terms are the half-spacing 2^-25 of fp16 subnormals for x's lo piece, and 2^-25 2^-10 for the scaled w's)
      bf16  2^-16 mag + K 2^-120"""
    xa, wa = x.to(torch.float64).abs(), w.to(torch.float64).abs()
    mag = xa @ wa.t()
    if pieces == "f16":
        return 2.0 ** -20 * mag + 2.0 ** -25 * wa.sum(-1) + 2.0 ** -35 * xa.sum(-1, keepdim=True)
    return 2.0 ** -16 * mag + x.shape[-1] * 2.0 ** -120


def check_split_domain(named: Iterable, where: str) -> None:
    """(name, matrix) pairs: a matrix with max|w| >= 64 has no fp16 pieces after the 2^10 scale -> ValueError naming it"""
    for name, w in named:
        m = float(w.detach().abs().max()) if w.numel() else 0.0
        if not m < SPLIT_W_LIMIT:
            raise ValueError(f"{where}: tower_arithmetic 'split' needs |w| < {SPLIT_W_LIMIT:g} in every matrix (fp16 pieces of 2^10 w), "
                             f"but {name} has max|w| = {m:g}; use tower_arithmetic 'exact'")


def pack_split_weight(w: torch.Tensor, pieces: int) -> torch.Tensor:
    """a contiguous fp32 device matrix [Nout, K] -> its packed pieces (uint8 buffer), `pieces` = hip.SPLIT_F16 | hip.SPLIT_BF16"""
    from . import hip
    lib = hip.lib()
    assert w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous()
    nout, k = w.shape
    out = torch.empty(int(lib.ssr_linear_split_pack_bytes(nout, k)), dtype=torch.uint8, device=w.device)
    hip.check(lib.ssr_linear_split_pack(w.data_ptr(), nout, k, pieces, out.data_ptr(), hip.stream_ptr()), "ssr_linear_split_pack")
    return out


def pack_tower(w: Dict[str, torch.Tensor], forward: Iterable[str], transposed: Iterable[str] = ()) -> None:
    """In place: `<key>.pk` = the fp16-piece pack of w[key] for every key of `forward`, `<key>.t.pk` = the bf16-piece pack of
    w[key]^T for every key of `transposed` (the transposed fp32 copy is a temporary)."""
    from . import hip
    for key in forward:
        w[f"{key}.pk"] = pack_split_weight(w[key], hip.SPLIT_F16)
    for key in transposed:
        w[f"{key}.t.pk"] = pack_split_weight(w[key].t().contiguous(), hip.SPLIT_BF16)
