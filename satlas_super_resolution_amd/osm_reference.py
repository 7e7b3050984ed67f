"""The object branch of OSMObjDiscriminator stated in plain torch for the CPU: what csrc/attention.hip and engine.ObjectBranchPlan are
tested against, and what runs without a GPU.  Written from the behaviour of the reference's network (ssr/archs/
osm_obj_discriminator_arch.py:8-31 SelfAttentionBlock, :49-54 and :74-79 the object branch), not from its text.

    attention_forward(x, p)                    token form: x [B, N, C] -> (y, saved);  p = dict(wq, bq, wk, bk, wv, bv, gamma)
    attention_backward(dy, x, p, saved)        the closed-form backward -> dict(dx, dwq, dbq, dwk, dbk, dwv, dbv, dgamma)
    self_attention(x, p)                       NCHW, differentiable THROUGH the closed form above (an autograd.Function)
    object_branch(sd, osm_objs)                o_out of the network from a state_dict; differentiable, any float dtype
    attention_params(sd, prefix)               the dict `p` of one block from a state_dict

and the object crops of OSMObjESRGANModel (ssr/models/osm_objs_esrgan_model.py:166-200), what csrc/obj_crop.hip and the model's host
side are tested against:

    resize_taps(n_in, n_out, antialias)        the tap rule of the bilinear resize, per output: (first, count, weights)
    resize_matrix(n_in, n_out, antialias)      the same as a dense [n_out, n_in] matrix
    crop_resize_reference(img, boxes, aa)      [Bo, C, 32, 32] crops of img [B, C, H, W] for boxes (b, x1, y1, x2, y2); differentiable
    crop_resize_backward(g, boxes, shape, aa)  its closed-form gradient w.r.t. img (the transpose)
    fix_box(box) / resolve_boxes(...)          the reference's repair of degenerate boxes, then Python slice semantics
    flatten_objects(chip_objs)                 the boxes of one chip in dict order, then list order
    sample_objects(chip_objs, n, rng=random)   the indices the reference keeps, consuming `rng` exactly as it does

Token order is the reference's view(B, -1, W * H): token i = h * W + w.  Every function computes in the dtype of its inputs: pass
float64 tensors for the float64 statement.
"""
from __future__ import annotations

import random
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F

ATTN_GRADS = ("dx", "dwq", "dbq", "dwk", "dbk", "dwv", "dbv", "dgamma")


def attention_params(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """query_conv / key_conv / value_conv are 1 x 1 convolutions: their weights as [out, in] matrices"""
    m = lambda k: sd[f"{prefix}.{k}.weight"].flatten(1)
    return dict(wq=m("query_conv"), bq=sd[f"{prefix}.query_conv.bias"], wk=m("key_conv"), bk=sd[f"{prefix}.key_conv.bias"],
                wv=m("value_conv"), bv=sd[f"{prefix}.value_conv.bias"], gamma=sd[f"{prefix}.gamma"])


def attention_forward(x: torch.Tensor, p: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    q = x @ p["wq"].t() + p["bq"]                              # [B, N, dk]
    k = x @ p["wk"].t() + p["bk"]
    v = x @ p["wv"].t() + p["bv"]                              # [B, N, C]
    e = q @ k.transpose(1, 2)                                  # e[i][j] = q_i . k_j
    a = torch.softmax(e, dim=2)                                # over the keys
    out = a @ v
    return p["gamma"] * out + x, dict(a=a, q=q, k=k, v=v, out=out)


def attention_backward(dy: torch.Tensor, x: torch.Tensor, p: Dict[str, torch.Tensor], s: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    g = p["gamma"]
    dgamma = (dy * s["out"]).sum().reshape(1)
    dout = g * dy
    dv = s["a"].transpose(1, 2) @ dout
    da = dout @ s["v"].transpose(1, 2)
    de = s["a"] * (da - (s["a"] * da).sum(dim=2, keepdim=True))     # softmax backward, row by row
    dq = de @ s["k"]
    dk = de.transpose(1, 2) @ s["q"]
    dx = dy + dq @ p["wq"] + dk @ p["wk"] + dv @ p["wv"]            # the residual path first
    tok = lambda t: t.reshape(-1, t.shape[-1])
    return dict(dx=dx, dgamma=dgamma,
                dwq=tok(dq).t() @ tok(x), dbq=tok(dq).sum(0), dwk=tok(dk).t() @ tok(x), dbk=tok(dk).sum(0),
                dwv=tok(dv).t() @ tok(x), dbv=tok(dv).sum(0))


class _SelfAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, gamma):
        p = dict(wq=wq, bq=bq, wk=wk, bk=bk, wv=wv, bv=bv, gamma=gamma)
        y, s = attention_forward(x, p)
        ctx.save_for_backward(x, wq, bq, wk, bk, wv, bv, gamma, s["a"], s["q"], s["k"], s["v"], s["out"])
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wq, bq, wk, bk, wv, bv, gamma, a, q, k, v, out = ctx.saved_tensors
        g = attention_backward(dy, x, dict(wq=wq, bq=bq, wk=wk, bk=bk, wv=wv, bv=bv, gamma=gamma), dict(a=a, q=q, k=k, v=v, out=out))
        return g["dx"], g["dwq"], g["dbq"], g["dwk"], g["dbk"], g["dwv"], g["dbv"], g["dgamma"]


def to_tokens(x: torch.Tensor) -> torch.Tensor:
    """NCHW -> [B, H * W, C]"""
    return x.flatten(2).transpose(1, 2)


def self_attention(x: torch.Tensor, p: Dict[str, torch.Tensor]) -> torch.Tensor:
    B, C, H, W = x.shape
    y = _SelfAttentionFn.apply(to_tokens(x), p["wq"], p["bq"], p["wk"], p["bk"], p["wv"], p["bv"], p["gamma"])
    return y.transpose(1, 2).reshape(B, C, H, W)


def object_branch(sd: Dict[str, torch.Tensor], osm_objs: torch.Tensor, return_attention: bool = False):
    """o_out [Bo, 1, H / 16, W / 16] of the network for osm_objs [Bo, 3, H, W]; with return_attention also the two attention matrices"""
    conv = lambda name, t: F.conv2d(t, sd[name + ".weight"], sd[name + ".bias"], stride=2, padding=1)
    o1 = torch.relu(conv("o_conv1", osm_objs))
    o2 = torch.relu(conv("o_conv2", o1))
    p1, p2 = attention_params(sd, "o_attention1"), attention_params(sd, "o_attention2")
    a1 = self_attention(o2, p1)
    o3 = torch.relu(conv("o_conv3", a1))
    a2 = self_attention(o3, p2)
    o_out = torch.relu(conv("o_conv4", a2))
    if return_attention:
        with torch.no_grad():
            return o_out, (attention_forward(to_tokens(o2), p1)[1]["a"], attention_forward(to_tokens(o3), p2)[1]["a"])
    return o_out


# =====================================================================================================
# Object crops of OSMObjESRGANModel
# =====================================================================================================
OBJ_CROP = 32             # every crop is resized to 32 x 32 (osm_objs_esrgan_model.py:180-181)
FIX_LIMIT = 128           # the literal of the fix-up at :173-176: the reference's own, whatever the image size


def resize_taps(n_in: int, n_out: int = OBJ_CROP, antialias: bool = False) -> List[Tuple[int, int, List[float]]]:
    """torchvision.transforms.functional.resize of a float tensor (bilinear, align_corners=False) along one axis: for every output
    i the first source index, the number of taps and their weights (Python floats = float64), normalised to sum 1.  Without
    antialiasing, or when enlarging, the support is one source pixel (at most 2 taps); with it and scale >= 1 the triangle is `scale`
    wide (at most 8 taps at 128 -> 32)."""
    scale = n_in / n_out
    support = scale if (antialias and scale >= 1.0) else 1.0
    out = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n_in) - first
        w = [max(0.0, 1.0 - abs((j + first - center + 0.5) / support)) for j in range(count)]
        total = sum(w)
        out.append((first, count, [v / total for v in w]))
    return out


def resize_matrix(n_in: int, n_out: int = OBJ_CROP, antialias: bool = False, dtype=torch.float64) -> torch.Tensor:
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i, (first, count, w) in enumerate(resize_taps(n_in, n_out, antialias)):
        m[i, first:first + count] = torch.tensor(w, dtype=torch.float64)
    return m.to(dtype)


def crop_resize_reference(img: torch.Tensor, boxes: Sequence[Sequence[int]], antialias: bool = False) -> torch.Tensor:
    """img [B, C, H, W], boxes (b, x1, y1, x2, y2) already fixed up and slice-resolved -> [Bo, C, 32, 32] in img's dtype; the 2-D weight
    is the product of the two axes' weights.  Plain tensor algebra: autograd differentiates it."""
    out = []
    for b, x1, y1, x2, y2 in boxes:
        my = resize_matrix(y2 - y1, OBJ_CROP, antialias, img.dtype)
        mx = resize_matrix(x2 - x1, OBJ_CROP, antialias, img.dtype)
        out.append(my @ img[b, :, y1:y2, x1:x2] @ mx.t())
    return torch.stack(out)


def crop_resize_backward(g: torch.Tensor, boxes: Sequence[Sequence[int]], shape: Sequence[int], antialias: bool = False) -> torch.Tensor:
    """the gradient of sum(crop_resize_reference(img) * g) w.r.t. img of `shape` [B, C, H, W]: every box adds My^T g Mx to its window"""
    d = torch.zeros(*shape, dtype=g.dtype)
    for o, (b, x1, y1, x2, y2) in enumerate(boxes):
        my = resize_matrix(y2 - y1, OBJ_CROP, antialias, g.dtype)
        mx = resize_matrix(x2 - x1, OBJ_CROP, antialias, g.dtype)
        d[b, :, y1:y2, x1:x2] += my.t() @ g[o] @ mx
    return d


def fix_box(box: Sequence[int]) -> Tuple[int, int, int, int]:
    """osm_objs_esrgan_model.py:173-176: a box of zero width / height is widened by one pixel, to the right / downwards unless its far
    edge is at 128 or beyond"""
    x1, y1, x2, y2 = (int(v) for v in box)
    if x1 == x2:
        x1, x2 = (x1, x2 + 1) if x2 < FIX_LIMIT else (x1 - 1, x2)
    if y1 == y2:
        y1, y2 = (y1, y2 + 1) if y2 < FIX_LIMIT else (y1 - 1, y2)
    return x1, y1, x2, y2


def flatten_objects(chip_objs: Dict[str, Sequence[Sequence[int]]]) -> List[Sequence[int]]:
    """:168-169: every box of a chip in dict order, then list order"""
    return [o for v in chip_objs.values() for o in v]


def resolve_boxes(objs: Sequence[Sequence[int]], H: int, W: int, chip: str = "?") -> List[Tuple[int, int, int, int]]:
    """fix_box, then `[:, y1:y2, x1:x2]` under Python slice semantics (negative and over-long indices as slice.indices resolves
    them) -> (x1, y1, x2, y2) with 0 <= x1 < x2 <= W, 0 <= y1 < y2 <= H.  An empty crop, on which the reference's resize crashes,
    raises ValueError naming the chip."""
    out = []
    for i, o in enumerate(objs):
        x1, y1, x2, y2 = fix_box(o)
        ys, ye, _ = slice(y1, y2).indices(H)
        xs, xe, _ = slice(x1, x2).indices(W)
        if ye <= ys or xe <= xs:
            raise ValueError(f"chip {chip!r}: object {i} with box {list(o)} is an empty crop of a {H} x {W} image")
        out.append((xs, ys, xe, ye))
    return out


def sample_objects(chip_objs: Dict[str, Sequence[Sequence[int]]], n: int, rng=random) -> List[int]:
    """:195-198: random.sample over the index list, once per image; the chosen objects stay in ascending index order.  Fewer than n
    objects: random.sample's own ValueError."""
    total = len(flatten_objects(chip_objs))
    picked = rng.sample([i for i in range(0, total)], n)
    return [g for g in range(total) if g in picked]
