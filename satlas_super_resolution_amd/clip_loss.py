"""The CLIP loss of `train.clip_opt` (the reference's ssr/losses/basic_loss.py:19-48, called at ssr_esrgan_model.py:187-190 with
(self.output, l1_gt)): an L1 distance between the pooled features that a frozen vision tower gives the generated image and the
target, back-propagated through the tower to the generated image.

    x, gt      = F.interpolate(., (S, S))                    default mode 'nearest'; float images in [0, 1], RGB, no / 255
    x, gt      = (. - OPENAI_MEAN) / OPENAI_STD              OpenAI's mean / std even for a SigLIP tower: the reference's text, kept
    fx, fg     = encode_image(x), encode_image(gt)           open_clip, normalize=False [recalled]: the raw pooled features [B, E]
    l_clip_sim = loss_weight * mean(|fx - fg|)               reduction 'mean' over all B * E elements

The tower is the config-driven ViT of clipscore_metric.py (`ViT-B-16-SigLIP-256` is that family: width 768, depth 12, 12 heads of 64,
MLP 3072, patch 16, 256 tokens [recalled]); what is added here is its backward pass with respect to the IMAGE.  The tower's weights
are not trained, so no weight gradient exists anywhere.  Only the siglip family (no class token) has a backward; a `clip` tower is
refused by name.  Statements that rest on open_clip behaviour that cannot be executed here are marked [recalled].

    nearest_inverse_ranges     per source index, the half-open range of destination indices that F.interpolate('nearest') reads it for
    clip_loss_input            the nearest resize by nearest_index_table, then mean / std
    clip_loss_reference        the definition, differentiable (autograd), on clipscore_metric.vit_features_from_input
    clip_loss_grad_reference   the same loss and its image gradient in closed form, piece by piece as the kernels compute it
    check_clip_opt             the keys of a `train.clip_opt` block and its weights file (no device)
    ClipLossModel / ClipLossPlan     the weights (and their transposes) on the device / the static launch lists (vit_tower.py, csrc/vit_bwd.hip)

`tower_arithmetic` ('exact' | 'split') and `tower_attention` ('fma' | 'mfma') are the tower's own, orthogonal options (vit_tower.py).  Under
'split' the backward's transposes run as ssr_linear_split on bf16 pieces, which clip_loss_grad_reference restates on the CPU; under 'mfma'
the blocks' attention backward is ssr_mha_mfma_bwd: exact fp32 products in another order of additions, so the CPU statements hold unchanged.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

from .clipscore_metric import CLIP_MEAN, CLIP_STD, _GELUS, _attention, nearest_index_table, vit_config_from_state, vit_features_from_input
from .linear_split import check_tower_arithmetic, check_tower_attention, linear_split_reference
from .vit_tower import TowerPlan, TowerWeights

CLIP_LOSS_MODELS = {"ViT-B-16-SigLIP-256": "siglip"}                                 # the reference's clip_loss_model -> family
CLIP_LOSS_MEAN, CLIP_LOSS_STD = CLIP_MEAN["clip"], CLIP_STD["clip"]                    # OpenAI's, whatever the tower


# ---------------------------------------------------------------- the resize and its transpose
def nearest_inverse_ranges(n_in: int, n_out: int, used: int = None) -> torch.Tensor:
    """int64 [n_in, 2]: for every source index i the half-open range [lo, hi) of destination indices below `used` (default n_out) whose
    entry in nearest_index_table(n_in, n_out) is i.  The table is monotone (asserted), so the destinations of one source are
    contiguous; a source that nothing reads gets an empty range (lo == hi)."""
    table = nearest_index_table(n_in, n_out)
    used = n_out if used is None else used
    assert 0 <= used <= n_out
    assert bool((table[1:] >= table[:-1]).all()), "nearest_index_table is not monotone"
    t = table[:used].contiguous()
    i = torch.arange(n_in, dtype=torch.int64)
    lo = torch.searchsorted(t, i, right=False)
    hi = torch.searchsorted(t, i, right=True)
    return torch.stack([lo, hi], dim=1)


def _mean_std(dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    mean = torch.tensor(CLIP_LOSS_MEAN, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)      # float32 values on both sides
    std = torch.tensor(CLIP_LOSS_STD, dtype=torch.float32).to(dtype).view(1, 3, 1, 1)
    return mean, std


def clip_loss_input(img_nchw: torch.Tensor, size: int, dtype=torch.float64) -> torch.Tensor:
    """float [N, 3, H, W] in [0, 1] -> what the tower is fed, [N, 3, size, size]: the nearest resize (by the index tables, so autograd
    scatters back through them), then (x - mean) / std.  In float32 this is the operation order of ssr_vit_float_input."""
    assert img_nchw.dim() == 4 and img_nchw.shape[1] == 3, "float [N, 3, H, W]"
    rows, cols = nearest_index_table(img_nchw.shape[2], size), nearest_index_table(img_nchw.shape[3], size)
    x = img_nchw.to(dtype)[:, :, rows][:, :, :, cols]
    mean, std = _mean_std(dtype)
    return (x - mean) / std


def clip_loss_reference(fake: torch.Tensor, gt: torch.Tensor, state: Dict[str, torch.Tensor], loss_weight: float = 1.0, gelu: str = "tanh",
                        dtype=torch.float64) -> torch.Tensor:
    """l_clip_sim of float NCHW images; differentiable with respect to `fake`"""
    size = vit_config_from_state(state)["image_size"]
    fx = vit_features_from_input(clip_loss_input(fake, size, dtype), state, gelu)
    with torch.no_grad():
        fg = vit_features_from_input(clip_loss_input(gt, size, dtype), state, gelu)
    return loss_weight * (fx - fg).abs().mean()


# ---------------------------------------------------------------- the gradient in closed form
def _ln_bwd(x, w, dy, eps):
    """the backward of F.layer_norm over the last axis with respect to its input: with g = dy * w,
    dx = rstd * (g - mean(g) - xhat * mean(g * xhat))"""
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xhat, g = (x - mean) * rstd, dy * w
    return rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))


def _act_grad(v, gelu: str):
    """d/dv of F.gelu (siglip towers only)"""
    if gelu == "tanh":
        k = 0.7978845608028654
        t = torch.tanh(k * (v + 0.044715 * v ** 3))
        return 0.5 * (1 + t) + 0.5 * v * (1 - t * t) * k * (1 + 3 * 0.044715 * v * v)
    return 0.5 * (1 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327


def _attention_bwd(q, k, v, dy, heads: int):
    """q, dy [N, Tq, C], k, v [N, Tk, C] -> dq, dk, dv.  S = q k^T scale, P = softmax(S), dP = dy v^T, delta = sum_j P dP,
    dS = P (dP - delta): dv = P^T dy, dk = scale dS^T q, dq = scale dS k"""
    n, _, c = q.shape
    d = c // heads
    scale = d ** -0.5
    sp = lambda t: t.reshape(n, t.shape[1], heads, d).transpose(1, 2)          # noqa: E731
    qh, kh, vh, gh = sp(q), sp(k), sp(v), sp(dy)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    dp = gh @ vh.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    un = lambda t: t.transpose(1, 2).reshape(n, t.shape[2], c)                  # noqa: E731
    return un(ds @ kh * scale), un(ds.transpose(-1, -2) @ qh * scale), un(p.transpose(-1, -2) @ gh)


def clip_loss_grad_reference(fake: torch.Tensor, gt: torch.Tensor, state: Dict[str, torch.Tensor], loss_weight: float = 1.0,
                             gelu: str = "tanh", dtype=torch.float64, tower_arithmetic: str = "exact") -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (l_clip_sim, d l_clip_sim / d fake [N, 3, H, W]) without autograd: LayerNorm backward, softmax-attention backward, the
    activation derivative, the linear transposes, the pooling head with Tq = 1, and the transposed resize as a gather over the
    inverse index ranges - the pieces, and their order, of ClipLossPlan's backward.  tower_arithmetic 'split': every forward product
    (of both images) is linear_split_reference with fp16 pieces, every transpose with bf16 pieces, as ClipLossPlan launches them."""
    split = check_tower_arithmetic(tower_arithmetic, "tower_arithmetic") == "split"
    mm = (lambda t, w, b=None: linear_split_reference(t, w, b, "f16").to(dtype)) if split else F.linear                 # noqa: E731
    mt = (lambda dy, w: linear_split_reference(dy, w.t(), None, "bf16").to(dtype)) if split else (lambda dy, w: dy @ w)   # noqa: E731
    cfg = vit_config_from_state(state)
    if cfg["family"] != "siglip":
        raise NotImplementedError("train.clip_opt: the backward of a `clip` tower (class token) is not built: no clip_loss_model needs it")
    heads, eps, Cw, p, g, S = cfg["heads"], cfg["ln_eps"], cfg["width"], cfg["patch"], cfg["grid"], cfg["image_size"]
    Wt = lambda k: state[k].to(dtype)                                          # noqa: E731
    lin = lambda t, name: mm(t, Wt(f"{name}.weight"), Wt(f"{name}.bias"))       # noqa: E731
    ln = lambda t, name: F.layer_norm(t, (Cw,), Wt(f"{name}.weight"), Wt(f"{name}.bias"), eps)       # noqa: E731
    act = lambda t: F.gelu(t, approximate="tanh" if gelu == "tanh" else "none")  # noqa: E731
    with torch.no_grad():
        fg = vit_features_from_input(clip_loss_input(gt, S, dtype), state, gelu, tower_arithmetic)
        N, _, H, W = fake.shape
        xin = clip_loss_input(fake, S, dtype)[:, :, :g * p, :g * p]
        patches = xin.reshape(N, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(N, g * g, 3 * p * p)
        x = mm(patches, Wt("patch.weight").reshape(Cw, -1), Wt("patch.bias")) + Wt("pos")
        saved = []
        for i in range(cfg["depth"]):
            b = f"blocks.{i}"
            qkv = lin(ln(x, f"{b}.ln1"), f"{b}.qkv")
            q, k, v = qkv.chunk(3, dim=-1)
            x_mid = x + lin(_attention(q, k, v, heads), f"{b}.proj")
            pre = lin(ln(x_mid, f"{b}.ln2"), f"{b}.fc1")
            saved.append((x, qkv, x_mid, pre))
            x = x_mid + lin(act(pre), f"{b}.fc2")
        pq = lin(Wt("pool.probe").expand(N, 1, -1), "pool.q")
        pk, pv = lin(ln(x, "ln_post"), "pool.kv").chunk(2, dim=-1)
        py = lin(_attention(pq, pk, pv, heads), "pool.proj")
        ppre = lin(ln(py, "pool.ln"), "pool.fc1")
        fx = (py + lin(act(ppre), "pool.fc2"))[:, 0]
        diff = fx - fg
        loss = loss_weight * diff.abs().mean()
        # backward
        df = (loss_weight / diff.numel() * torch.sign(diff))[:, None]                                   # [N, 1, C]
        dpre = mt(df, Wt("pool.fc2.weight")) * _act_grad(ppre, gelu)
        dpy = _ln_bwd(py, Wt("pool.ln.weight"), mt(dpre, Wt("pool.fc1.weight")), eps) + df
        _, dk, dv = _attention_bwd(pq, pk, pv, mt(dpy, Wt("pool.proj.weight")), heads)                    # the probe is a parameter: no dq
        dx = _ln_bwd(x, Wt("ln_post.weight"), mt(torch.cat([dk, dv], dim=-1), Wt("pool.kv.weight")), eps)
        for i in reversed(range(cfg["depth"])):
            b = f"blocks.{i}"
            x_in, qkv, x_mid, pre = saved[i]
            dpre = mt(dx, Wt(f"{b}.fc2.weight")) * _act_grad(pre, gelu)
            dx_mid = _ln_bwd(x_mid, Wt(f"{b}.ln2.weight"), mt(dpre, Wt(f"{b}.fc1.weight")), eps) + dx
            q, k, v = qkv.chunk(3, dim=-1)
            dqkv = torch.cat(_attention_bwd(q, k, v, mt(dx_mid, Wt(f"{b}.proj.weight")), heads), dim=-1)
            dx = _ln_bwd(x_in, Wt(f"{b}.ln1.weight"), mt(dqkv, Wt(f"{b}.qkv.weight")), eps) + dx_mid
        dpatch = mt(dx, Wt("patch.weight").reshape(Cw, -1))                                              # [N, G, 3 p p]
        dxin = dpatch.reshape(N, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(N, 3, g * p, g * p)
        # the transposed resize: every source pixel gathers the destinations of its row range x column range (prefix sums)
        rr, cr = nearest_inverse_ranges(H, S, g * p), nearest_inverse_ranges(W, S, g * p)
        cs = F.pad(dxin.cumsum(2), (0, 0, 1, 0))
        rows = cs[:, :, rr[:, 1]] - cs[:, :, rr[:, 0]]
        cs = F.pad(rows.cumsum(3), (1, 0))
        grad = (cs[:, :, :, cr[:, 1]] - cs[:, :, :, cr[:, 0]]) / _mean_std(dtype)[1]
    return loss, grad


# ---------------------------------------------------------------- the option block
CLIP_LOSS_REFUSED = {"EVA02-E-14-plus": "4.4 B parameters", "RN50": "a ResNet, not a vision transformer"}    # the reference's other two branches
CLIP_LOSS_ENV = "SSR_CLIP_LOSS_SIGLIP_B16_WEIGHTS"
CLIP_LOSS_PRETRAIN_PATH = "experiments/pretrained_models/clip_siglip_b16_256.pth"
_SAVE_HINT = "torch.save(open_clip.create_model_and_transforms('ViT-B-16-SigLIP-256', pretrained='webli')[0].visual.state_dict(), <file>)"
_CLIP_OPT_KEYS = ("type", "clip_loss_model", "loss_weight", "clip_weights", "gelu", "tower_arithmetic", "tower_attention")


def check_clip_opt(block: Dict) -> Dict:
    """Validates a `train.clip_opt` block and finds the weights -> {"model", "family", "path", "gelu", "loss_weight"}.  Touches no
    device.  Keys: type (CLIPLoss), clip_loss_model (ViT-B-16-SigLIP-256), loss_weight (default 1.0, as CLIPLoss.__init__); ours:
    clip_weights (a file), gelu ('tanh' | 'erf', default 'tanh' as the CLIPScore metric), tower_arithmetic ('exact', the default and
    what an absent key means: the result carries no such entry | 'split': "tower_arithmetic": "split"), tower_attention ('fma', the
    default, likewise absent from the result | 'mfma': "tower_attention": "mfma").  The weights file is the option
    `clip_weights`, else the environment variable SSR_CLIP_LOSS_SIGLIP_B16_WEIGHTS, else the default path; anything else raises
    NotImplementedError beginning `train.clip_opt`."""
    import os
    if block.get("type") != "CLIPLoss":
        raise NotImplementedError(f"train.clip_opt.type={block.get('type')!r}: only CLIPLoss")
    for k in block:
        if k not in _CLIP_OPT_KEYS:
            raise NotImplementedError(f"train.clip_opt.{k}: CLIPLoss takes {', '.join(_CLIP_OPT_KEYS[1:])}")
    name = block.get("clip_loss_model")
    if name in CLIP_LOSS_REFUSED:
        raise NotImplementedError(f"train.clip_opt.clip_loss_model={name!r} ({CLIP_LOSS_REFUSED[name]}) is outside the MI355X path "
                                  f"(have {sorted(CLIP_LOSS_MODELS)})")
    if name not in CLIP_LOSS_MODELS:
        raise NotImplementedError(f"train.clip_opt.clip_loss_model={name!r} is not supported: the reference offers "
                                  f"{sorted(CLIP_LOSS_MODELS) + sorted(CLIP_LOSS_REFUSED)}")
    gelu = block.get("gelu", "tanh")
    if gelu not in _GELUS:
        raise NotImplementedError(f"train.clip_opt.gelu={gelu!r} (have {list(_GELUS)})")
    out = {"model": name, "family": CLIP_LOSS_MODELS[name], "gelu": gelu, "loss_weight": float(block.get("loss_weight", 1.0))}
    if check_tower_arithmetic(block.get("tower_arithmetic"), "train.clip_opt.tower_arithmetic") == "split":
        out["tower_arithmetic"] = "split"
    if check_tower_attention(block.get("tower_attention"), "train.clip_opt.tower_attention") == "mfma":
        out["tower_attention"] = "mfma"
    given = block.get("clip_weights")
    if given:
        if not os.path.exists(given):
            raise FileNotFoundError(f"train.clip_opt: clip_weights={given!r} does not exist")
        return dict(out, path=os.path.abspath(given))
    for cand in (os.environ.get(CLIP_LOSS_ENV), CLIP_LOSS_PRETRAIN_PATH):
        if cand and os.path.exists(cand):
            return dict(out, path=os.path.abspath(cand))
    raise NotImplementedError(
        f"train.clip_opt: no weights found for clip_loss_model={name!r}.  Put them in one of three places: the option "
        f"`train.clip_opt.clip_weights: <file>`, the environment variable {CLIP_LOSS_ENV}=<file>, or {CLIP_LOSS_PRETRAIN_PATH}.  Save the "
        f"file with {_SAVE_HINT}.  There is no silent random network: a loss from random weights is not the CLIP loss")


# ---------------------------------------------------------------- the device path
_LOSS_MODELS: Dict[Tuple, "ClipLossModel"] = {}


def _loss_model_key(path: str, device, gelu: str, tower_arithmetic: str, tower_attention: str) -> Tuple:
    device = torch.device(device)
    return (path, device.type, device.index, gelu, tower_arithmetic, tower_attention)


def clip_loss_model(path: str, device, gelu: str = "tanh", tower_arithmetic: str = "exact", tower_attention: str = "fma") -> "ClipLossModel":
    """the tower of a weights file on the device, loaded once per (resolved path, device, gelu, tower_arithmetic, tower_attention)"""
    from .clipscore_metric import load_clip_visual_state
    key = _loss_model_key(path, device, gelu, tower_arithmetic, tower_attention)
    if key not in _LOSS_MODELS:
        _LOSS_MODELS[key] = ClipLossModel(load_clip_visual_state(path, "siglip"), torch.device(device), gelu, tower_arithmetic, tower_attention)
    return _LOSS_MODELS[key]


class ClipLossModel(TowerWeights):
    """A siglip tower's weights with what its backward reads (vit_tower.TowerWeights, backward=True); a `clip` tower is refused."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda", gelu: str = "tanh", tower_arithmetic: str = "exact",
                 tower_attention: str = "fma"):
        if gelu not in _GELUS:
            raise NotImplementedError(f"train.clip_opt: gelu={gelu!r} (have {list(_GELUS)})")
        tower_arithmetic = check_tower_arithmetic(tower_arithmetic, "train.clip_opt.tower_arithmetic")
        tower_attention = check_tower_attention(tower_attention, "train.clip_opt.tower_attention")
        if vit_config_from_state(state)["family"] != "siglip":
            raise NotImplementedError("train.clip_opt: the backward of a `clip` tower (class token) is not built: no clip_loss_model needs it")
        super().__init__(state, device, gelu, tower_arithmetic, tower_attention, "train.clip_opt", backward=True)


class ClipLossPlan(TowerPlan):
    """Static launch lists for B image pairs of H x W.  `fake_view` / `target_view` / `grad_view` are fp32 NHWC views (hip.View) of the
    generated images, the targets and the gradient image (B * H * W pixels, channels coff .. coff + 2 = RGB); `loss_ptr` a float
    scalar (slot 0 of a slotted buffer in deterministic mode) that l_clip_sim is ADDED to, as the other loss kernels do.

      fwd_target   the tower on the target rows into scratch: nothing is saved
      fwd_fake     the tower on the generated rows: per block x_in, the packed qkv, x_mid and the fc1 pre-activation stay
      bwd          ssr_feature_l1, the pooling head, ln_post, the blocks in reverse, the patch embedding, ssr_vit_float_input_bwd,
                   which ADDS the image gradient into grad_view
    `launcher` is the three in that order.  Both forwards are vit_tower.TowerPlan.forward behind ssr_vit_float_input with fc1's
    pre-activation kept, so the two feature sets come from identical arithmetic."""

    def __init__(self, model: ClipLossModel, B: int, H: int, W: int, fake_view, target_view, grad_view, loss_ptr: int, weight: float = 1.0,
                 flags: int = 0):
        from . import engine, hip
        from .hip import NULL_VIEW, view
        super().__init__(model, B, H, W, "the CLIP loss")
        cfg, dev, lib = model.cfg, model.device, self.lib
        Cw, p, g, T, mlp, heads, d, depth = (cfg[k] for k in ("width", "patch", "grid", "tokens", "mlp", "heads", "head_dim", "depth"))
        mfma = model.tower_attention == "mfma"                               # the blocks'; the pooling head keeps ssr_mha_bwd
        ws_floats, mha_bwd = (lib.ssr_mha_mfma_bwd_ws_floats, lib.ssr_mha_mfma_bwd) if mfma else (lib.ssr_mha_bwd_ws_floats, lib.ssr_mha_bwd)
        KP, M, scale, act, F32 = 3 * p * p, B * T, float(d) ** -0.5, model.act, hip.F32
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        self._perm = (C.c_int32 * 3)(0, 1, 2)
        self._mean, self._std = (C.c_float * 3)(*CLIP_LOSS_MEAN), (C.c_float * 3)(*CLIP_LOSS_STD)
        b = self.bufs = {"patches": z(M, KP), "embed": z(M, Cw), "h": z(M, Cw), "att": z(M, Cw), "post": z(M, mlp),
                         "probe": model.w["pool.probe"].reshape(1, Cw).repeat(B, 1).contiguous(), "pz": z(B, Cw), "pa": z(B, Cw), "pm": z(B, mlp),
                         # the target pass's scratch
                         "t.x": z(M, Cw), "t.qkv": z(M, 3 * Cw), "t.pre": z(M, mlp), "t.q": z(B, Cw), "t.kv": z(M, 2 * Cw), "t.py": z(B, Cw),
                         "t.ppre": z(B, mlp), "fg": z(B, Cw),
                         # what the generated rows keep
                         "q": z(B, Cw), "kv": z(M, 2 * Cw), "py": z(B, Cw), "ppre": z(B, mlp), "fx": z(B, Cw),
                         # gradients
                         "df": z(B, Cw), "dpm": z(B, mlp), "dpz": z(B, Cw), "dpy": z(B, Cw), "dpa": z(B, Cw), "dkv": z(M, 2 * Cw), "dh": z(M, Cw),
                         "dx": z(M, Cw), "dx2": z(M, Cw), "dmlp": z(M, mlp), "datt": z(M, Cw), "dqkv": z(M, 3 * Cw), "dpatch": z(M, KP),
                         # the blocks' attention backward sizes it; the pooling head's (Tq = 1, always ssr_mha_bwd) needs less
                         "ws": z(max(int(ws_floats(B, T, heads)), int(lib.ssr_mha_bwd_ws_floats(B, 1, heads)), 1))}
        for i in range(depth + 1):
            b[f"x.{i}"] = z(M, Cw)                                             # x.i: the input of block i; x.depth: the tower's last rows
        for i in range(depth):
            b[f"qkv.{i}"], b[f"xmid.{i}"], b[f"pre.{i}"] = z(M, 3 * Cw), z(M, Cw), z(M, mlp)
        self.saved_bytes = 4 * sum(b[k].numel() for k in b if k.split(".")[0] in ("x", "qkv", "xmid", "pre"))
        linear_t, layernorm_bwd, split = self.linear_t, self.layernorm_bwd, self.split

        def float_input(img):
            return lambda L, patches: L.add(lib.ssr_vit_float_input, img, B, H, W, self.rowidx.data_ptr(), self.colidx.data_ptr(), g, p, patches,
                                            F32, self._perm, self._mean, self._std, what="float input")

        self.fwd_target, self.fwd_fake, self.bwd = engine.Launcher(), engine.Launcher(), engine.Launcher()
        self.forward(self.fwd_target, float_input(target_view), b, [b["t.x"]] * (depth + 1), [b["t.qkv"]] * depth, [b["t.x"]] * depth,
                     [b["t.pre"]] * depth, (b["t.q"], b["t.kv"], b["t.py"], b["t.ppre"]), b["fg"])
        self.forward(self.fwd_fake, float_input(fake_view), b, [b[f"x.{i}"] for i in range(depth + 1)], [b[f"qkv.{i}"] for i in range(depth)],
                     [b[f"xmid.{i}"] for i in range(depth)], [b[f"pre.{i}"] for i in range(depth)], (b["q"], b["kv"], b["py"], b["ppre"]), b["fx"])

        L = self.bwd
        ws = b["ws"].data_ptr()
        L.add(lib.ssr_feature_l1, view(b["fx"]), view(b["fg"]), view(b["df"]), B, Cw, float(weight), loss_ptr, int(flags), what="feature l1")
        # the pooling head: f = py + fc2(act(fc1(ln(py)))), py = proj(attention(q(probe), kv(ln_post(x))))
        linear_t(L, view(b["df"]), "pool.fc2", view(b["dpm"]), B, Cw, mlp)
        L.add(lib.ssr_vit_act_bwd, view(b["ppre"]), view(b["dpm"]), view(b["dpm"]), F32, B, mlp, act, what="activation bwd pool")
        linear_t(L, view(b["dpm"]), "pool.fc1", view(b["dpz"]), B, mlp, Cw)
        layernorm_bwd(L, view(b["py"]), "pool.ln", view(b["dpz"]), view(b["df"]), view(b["dpy"]), B)
        linear_t(L, view(b["dpy"]), "pool.proj", view(b["dpa"]), B, Cw, Cw)
        ks, dks = split(b["kv"], 2), split(b["dkv"], 2)
        L.add(lib.ssr_mha_bwd, view(b["q"]), ks[0], ks[1], view(b["dpa"]), NULL_VIEW, dks[0], dks[1], ws, F32, B, 1, T, heads, d, scale,
              what="attention bwd pool")
        linear_t(L, view(b["dkv"]), "pool.kv", view(b["dh"]), M, 2 * Cw, Cw)
        layernorm_bwd(L, view(b[f"x.{depth}"]), "ln_post", view(b["dh"]), NULL_VIEW, view(b["dx"]), M)
        for i in reversed(range(depth)):
            n = f"blocks.{i}"
            linear_t(L, view(b["dx"]), f"{n}.fc2", view(b["dmlp"]), M, Cw, mlp)
            L.add(lib.ssr_vit_act_bwd, view(b[f"pre.{i}"]), view(b["dmlp"]), view(b["dmlp"]), F32, M, mlp, act, what=f"activation bwd {n}")
            linear_t(L, view(b["dmlp"]), f"{n}.fc1", view(b["dh"]), M, mlp, Cw)
            layernorm_bwd(L, view(b[f"xmid.{i}"]), f"{n}.ln2", view(b["dh"]), view(b["dx"]), view(b["dx2"]), M)
            linear_t(L, view(b["dx2"]), f"{n}.proj", view(b["datt"]), M, Cw, Cw)
            qs, dqs = split(b[f"qkv.{i}"], 3), split(b["dqkv"], 3)
            L.add(mha_bwd, qs[0], qs[1], qs[2], view(b["datt"]), dqs[0], dqs[1], dqs[2], ws, F32, B, T, T, heads, d, scale,
                  what=f"attention bwd {n}")
            linear_t(L, view(b["dqkv"]), f"{n}.qkv", view(b["dh"]), M, 3 * Cw, Cw)
            layernorm_bwd(L, view(b[f"x.{i}"]), f"{n}.ln1", view(b["dh"]), view(b["dx2"]), view(b["dx"]), M)
        # the position embedding adds a constant: the token gradient is the embedding's
        linear_t(L, view(b["dx"]), "patch", view(b["dpatch"]), M, Cw, KP)
        L.add(lib.ssr_vit_float_input_bwd, view(b["dpatch"]), B, H, W, self.rowrange.data_ptr(), self.colrange.data_ptr(), g, p, grad_view, F32,
              self._perm, self._std, what="float input bwd")
        self.launcher = engine.Launcher()
        for part in (self.fwd_target, self.fwd_fake, self.bwd):
            self.launcher.calls.extend(part.calls)
        self.features_fake, self.features_target = b["fx"], b["fg"]

    def run(self):
        self.launcher.run()
