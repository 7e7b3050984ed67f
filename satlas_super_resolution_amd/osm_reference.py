"""The object branch of OSMObjDiscriminator stated in plain torch for the CPU: what csrc/attention.hip and engine.ObjectBranchPlan are
tested against, and what runs without a GPU.  Written from the behaviour of the reference's network (ssr/archs/
osm_obj_discriminator_arch.py:8-31 SelfAttentionBlock, :49-54 and :74-79 the object branch), not from its text.

    attention_forward(x, p)                    token form: x [B, N, C] -> (y, saved);  p = dict(wq, bq, wk, bk, wv, bv, gamma)
    attention_backward(dy, x, p, saved)        the closed-form backward -> dict(dx, dwq, dbq, dwk, dbk, dwv, dbv, dgamma)
    self_attention(x, p)                       NCHW, differentiable THROUGH the closed form above (an autograd.Function)
    object_branch(sd, osm_objs)                o_out of the network from a state_dict; differentiable, any float dtype
    attention_params(sd, prefix)               the dict `p` of one block from a state_dict

Token order is the reference's view(B, -1, W * H): token i = h * W + w.  Every function computes in the dtype of its inputs: pass
float64 tensors for the float64 statement.
"""
from __future__ import annotations

from typing import Dict, Tuple

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
