"""The CLIPScore validation metric of the shipped option files (`clipscore: {type: calculate_clipscore, clip_model:
siglip-ViT-SO400M-14}`; the reference's ssr/metrics/clipscore.py:9-38) on the device.

The reference is 38 lines around the third-party `clip` and `open_clip` packages, which are not dependencies of this package.  What is
built here are the two vision towers those packages construct, written from their definitions and NOT executed against the packages
themselves: every statement below that rests on a package that cannot be executed here is marked [recalled] ("CLIPScore
metric").  The towers were cross-checked against the independent plain-torch statements of the `transformers` package
(SiglipVisionModel, CLIPVisionModelWithProjection) in float64; tools/make_clipscore_golden.py records that.

    score(a, b) = cos(f(a), f(b)),   f = model.encode_image(F.interpolate(img / 255, img_size))          (mode 'nearest', the default)
    cos(x, y)   = x . y / max(|x| |y|, 1e-8)                                   (torch <= 1.11's form; later ones differ below 1e-8 [recalled])

Three quirks of the reference are the defaults here, because users compare against numbers produced that way:
  * it is called with what `tensor2img` returns, which is BGR [recalled], so the tower's channel 0 sees blue (`rgb: true` undoes it);
  * it scales by /255 only: the tower sees raw [0, 1] values without its mean / std (`normalize: true` applies them: OpenAI's for
    `clip`, 0.5 / 0.5 for `siglip` [recalled]);
  * it resizes with F.interpolate's default mode, 'nearest', not the bicubic of the towers' own preprocessing.

One config-driven tower serves both families; the config is read off the weight shapes (vit_config_from_state), as clip.build_model
does [recalled], so nothing about "SO400M" or "B/16" is written down here and a two-layer test tower runs the same code.

                 siglip (timm VisionTransformer, global_pool='map') [recalled]    clip (OpenAI VisionTransformer) [recalled]
    patch embed  conv p x p stride p WITH bias                                    conv, NO bias
    tokens       grid^2 (no class token) + learned pos                            class token + grid^2, + learned pos, then ln_pre
    block        x += attn(ln1(x)); x += mlp(ln2(x)), packed qkv with bias        the same
    LN eps       1e-6                                                             1e-5
    activation   GELU, `gelu: tanh | erf` (below)                                 QuickGELU x * sigmoid(1.702 x)
    heads        the `heads` entry of the flat state (loader: 16 at width 1152,   width / 64
                 else width / 64); the head count cannot be read from shapes
    pooling      final LN, then the MAP head: one learned probe attends over all  ln_post(x[:, 0]) @ proj
                 tokens (MHA), y = a + mlp(ln(a)), output y[:, 0]; no projection
    real sizes   width 1152, depth 27, MLP 4304, patch 14, 729 tokens, out 1152   width 768, depth 12, MLP 3072, patch 16, 197 tokens, out 512

The SigLIP activation is the one open fact: the checkpoint was trained with the tanh approximation (`gelu_pytorch_tanh` in the
`transformers` config), and which one the reference's unpinned open_clip_torch / timm resolve to cannot be checked here; the default
is `tanh` [recalled] and the metric option `gelu: erf` selects the exact form (INTEGRATION.md says which to pick for a given timm).

Arithmetic: exact fp32 whatever the model's compute_dtype (a reported number, as LPIPS).  open_clip computes in fp32; `clip.load` on
a GPU computes in fp16 [recalled], so its numbers carry fp16 rounding that this path does not reproduce.  Weights stored as fp16 are
widened to fp32 on load.

    vit_config_from_state            the tower's sizes from the flat state's shapes
    load_clip_visual_state           open_clip / timm, transformers and OpenAI layouts (plain or TorchScript) -> the flat layout
    clip_random_state                random weights of any size (tests, throughput runs)
    nearest_index_table              F.interpolate(mode='nearest')'s source index per destination index, from F.interpolate itself
    clip_image_features_reference    the definition in torch on the CPU;   clipscore_reference   the same, for the score
    CLIPVisualModel / CLIPVisualPlan the weights on the device / the static launch list of one (B, H, W) (vit_tower.py, csrc/vit.hip)
    clipscore                        uint8 NHWC device images -> float64 [N] on the host
    check_clipscore_opt / calculate_clipscore        the entries of metrics.METRIC_CHECKS / metrics.METRICS

The flat layout: patch.weight [C, 3, p, p] (patch.bias), cls [C] (clip), pos [T, C], ln_pre.* (clip), blocks.{i}.{ln1, qkv, proj,
ln2, fc1, fc2}.{weight, bias}, ln_post.*, heads and image_size (int64 scalars); siglip: pool.probe [C], pool.{q, kv, proj, ln, fc1, fc2}.*; clip:
proj [C, E].
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .linear_split import check_tower_arithmetic, check_tower_attention, linear_split_reference
from .vit_tower import TowerPlan, TowerWeights

CLIP_MODELS = {"siglip-ViT-SO400M-14": "siglip", "clip-ViT-B/16": "clip"}          # the reference's names -> family
CLIP_REFUSED = ("clipa-ViT-bigG-14",)                                                # the reference's third branch: 1.8 B parameters
CLIP_IMG_SIZE = {"siglip": 384, "clip": 224}
CLIP_PRETRAIN_PATH = {"siglip": "experiments/pretrained_models/clip_siglip_so400m_14_384.pth",
                      "clip": "experiments/pretrained_models/clip_vit_b16.pt"}
CLIP_ENV = {"siglip": "SSR_CLIP_SIGLIP_WEIGHTS", "clip": "SSR_CLIP_VITB16_WEIGHTS"}
CLIP_MEAN = {"siglip": (0.5, 0.5, 0.5), "clip": (0.48145466, 0.4578275, 0.40821073)}     # [recalled]
CLIP_STD = {"siglip": (0.5, 0.5, 0.5), "clip": (0.26862954, 0.26130258, 0.27577711)}     # [recalled]
LN_EPS = {"siglip": 1e-6, "clip": 1e-5}
COS_EPS = 1e-8
_IGNORED_KEYS = ("crop_border", "test_y_channel", "input_order", "better", "type")
_OUR_KEYS = ("clip_weights", "rgb", "normalize", "gelu", "tower_arithmetic", "tower_attention")
_GELUS = ("tanh", "erf")
_BLOCK_LEAVES = ("ln1", "qkv", "proj", "ln2", "fc1", "fc2")
_POOL_LEAVES = ("q", "kv", "proj", "ln", "fc1", "fc2")


def _family(family: str) -> str:
    if family not in ("siglip", "clip"):
        raise ValueError(f"family {family!r}: 'siglip' or 'clip'")
    return family


def _default_heads(width: int) -> int:
    return 16 if width == 1152 else max(width // 64, 1)


def _default_image_size(family: str, patch: int, grid: int) -> int:
    """the reference's img_size for the family where the patch convolution (no padding: trailing pixels that do not fill a patch are
    dropped, 384 = 27 * 14 + 6) cuts it into this grid, else the grid's own size"""
    return CLIP_IMG_SIZE[family] if CLIP_IMG_SIZE[family] // patch == grid else grid * patch


def _int_entry(state, key: str, default: int) -> int:
    v = state.get(key)
    return int(v) if v is not None and not getattr(v, "is_meta", False) else default


# ---------------------------------------------------------------- config and weights
def vit_config_from_state(state: Dict[str, torch.Tensor]) -> Dict:
    """the tower's sizes from the SHAPES of a flat state (meta tensors will do): width from the patch embedding, patch size from its
    kernel, depth from the block count, token grid from the position embedding, MLP width from fc1, heads and image_size (the side
    the images are resized to, >= grid * patch) from the entries of those names, where present, else by the loader's rule"""
    for k in ("patch.weight", "pos"):
        if k not in state:
            raise KeyError(k)
    family = "siglip" if "pool.probe" in state else "clip"
    width, _, p, p2 = state["patch.weight"].shape
    if p != p2:
        raise ValueError(f"patch.weight: square patches only, got {tuple(state['patch.weight'].shape)}")
    depth = 1 + max((int(m.group(1)) for m in (re.match(r"blocks\.(\d+)\.", k) for k in state) if m), default=-1)
    if depth < 1 or "blocks.0.fc1.weight" not in state:
        raise KeyError("blocks.0.fc1.weight")
    tokens = state["pos"].shape[0]
    ncls = 1 if family == "clip" else 0
    grid = int(round((tokens - ncls) ** 0.5))
    if grid * grid + ncls != tokens or tuple(state["pos"].shape) != (tokens, width):
        raise ValueError(f"pos: shape {tuple(state['pos'].shape)} is no square token grid of width {width}" + (" behind a class token" if ncls else ""))
    heads = _int_entry(state, "heads", _default_heads(width))
    image_size = _int_entry(state, "image_size", _default_image_size(family, p, grid))
    if image_size // p != grid:
        raise ValueError(f"image_size = {image_size} is not cut into a {grid} x {grid} grid by {p} x {p} patches")
    if width % heads or (width // heads) % 8:
        raise ValueError(f"heads = {heads} does not divide width {width} into head dims that are multiples of 8")
    if family == "clip" and "proj" not in state:
        raise KeyError("proj")
    return {"family": family, "width": width, "patch": p, "depth": depth, "grid": grid, "tokens": tokens, "mlp": state["blocks.0.fc1.weight"].shape[0],
            "heads": heads, "head_dim": width // heads, "out_dim": width if family == "siglip" else state["proj"].shape[1],
            "image_size": image_size, "ln_eps": LN_EPS[family], "class_token": bool(ncls)}


def _flat_keys(family: str, depth: int):
    keys = ["patch.weight", "pos", "ln_post.weight", "ln_post.bias"]
    keys += ["patch.bias", "pool.probe"] if family == "siglip" else ["cls", "ln_pre.weight", "ln_pre.bias", "proj"]
    keys += [f"blocks.{i}.{leaf}.{wb}" for i in range(depth) for leaf in _BLOCK_LEAVES for wb in ("weight", "bias")]
    if family == "siglip":
        keys += [f"pool.{leaf}.{wb}" for leaf in _POOL_LEAVES for wb in ("weight", "bias")]
    return keys


def clip_random_state(family: str, seed: int = 0, width: Optional[int] = None, depth: Optional[int] = None, mlp: Optional[int] = None,
                      patch: Optional[int] = None, grid: Optional[int] = None, heads: Optional[int] = None,
                      out_dim: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Flat layout with random weights; the defaults are the real sizes of the family.  Matrices from N(0, 1 / fan_in), LayerNorm
    weights near 1, small biases: activations stay O(1) through the depth."""
    family = _family(family)
    real = {"siglip": (1152, 27, 4304, 14, 27, 16, 1152), "clip": (768, 12, 3072, 16, 14, 12, 512)}[family]
    width, depth, mlp, patch, grid = (v if v is not None else r for v, r in zip((width, depth, mlp, patch, grid), real))
    heads = heads if heads is not None else _default_heads(width)
    out_dim = out_dim if out_dim is not None else (width if family == "siglip" else real[6] if width == real[0] else width // 4)
    g = torch.Generator().manual_seed(seed)
    mat = lambda o, i: torch.randn(o, i, generator=g) / i ** 0.5                     # noqa: E731
    vec = lambda n, s=0.02: torch.randn(n, generator=g) * s                          # noqa: E731
    ncls = 0 if family == "siglip" else 1
    sd = {"patch.weight": torch.randn(width, 3, patch, patch, generator=g) / (3 * patch * patch) ** 0.5 * 2,
          "pos": torch.randn(grid * grid + ncls, width, generator=g) * 0.5}

    def lin(name, o, i):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = mat(o, i), vec(o)

    def ln(name):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = 1 + vec(width, 0.05), vec(width, 0.05)

    if family == "siglip":
        sd["patch.bias"] = vec(width)
    else:
        sd["cls"] = torch.randn(width, generator=g) * 0.5
        ln("ln_pre")
    for i in range(depth):
        ln(f"blocks.{i}.ln1"); lin(f"blocks.{i}.qkv", 3 * width, width); lin(f"blocks.{i}.proj", width, width)       # noqa: E702
        ln(f"blocks.{i}.ln2"); lin(f"blocks.{i}.fc1", mlp, width); lin(f"blocks.{i}.fc2", width, mlp)                # noqa: E702
    ln("ln_post")
    if family == "siglip":
        sd["pool.probe"] = torch.randn(width, generator=g)
        lin("pool.q", width, width); lin("pool.kv", 2 * width, width); lin("pool.proj", width, width)                # noqa: E702
        ln("pool.ln"); lin("pool.fc1", mlp, width); lin("pool.fc2", width, mlp)                                        # noqa: E702
    else:
        sd["proj"] = torch.randn(width, out_dim, generator=g) / width ** 0.5
    sd["heads"] = torch.tensor(heads)
    sd["image_size"] = torch.tensor(_default_image_size(family, patch, grid))
    return sd


def _torch_load(path: str) -> Dict[str, torch.Tensor]:
    """a state_dict from a plain checkpoint or, failing that, from a TorchScript archive (OpenAI's ViT-B-16.pt is one [recalled])"""
    try:
        sd = torch.load(path, map_location="cpu")
    except Exception as first:
        try:
            sd = torch.jit.load(path, map_location="cpu").state_dict()
        except Exception as second:
            raise ValueError(f"{path}: neither torch.load ({type(first).__name__}: {first}) nor torch.jit.load "
                             f"({type(second).__name__}: {second}) can read it") from first
    if hasattr(sd, "state_dict") and not isinstance(sd, dict):
        sd = sd.state_dict()
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return sd


_PREFIXES = ("visual.trunk.", "vision_model.", "visual.", "trunk.")         # longest first
# per source layout: flat block leaf -> source leaf
_TIMM_BLOCK = {"ln1": "norm1", "qkv": "attn.qkv", "proj": "attn.proj", "ln2": "norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
_OPENAI_BLOCK = {"ln1": "ln_1", "proj": "attn.out_proj", "ln2": "ln_2", "fc1": "mlp.c_fc", "fc2": "mlp.c_proj"}
_HF_BLOCK = {"ln1": "layer_norm1", "proj": "self_attn.out_proj", "ln2": "layer_norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}


def load_clip_visual_state(path, family: str) -> Dict[str, torch.Tensor]:
    """-> the flat layout (module docstring), float32, from a file (or an already loaded state_dict) in any of these layouts:
      * siglip, open_clip / timm state_dict, with or without the `visual.trunk.` prefix: patch_embed.proj, pos_embed, blocks.N.{norm1,
        attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2}, norm, attn_pool.{latent, q, kv, proj, norm, mlp.fc1, mlp.fc2}          [recalled]
      * siglip, transformers' SiglipVisionModel: separate q / k / v projections, head.probe, head.attention.in_proj_*
      * clip, OpenAI's file as a plain state_dict or as the TorchScript archive, with or without the `visual.` prefix       [recalled]
      * clip, transformers' CLIPVisionModelWithProjection: `pre_layrnorm` as spelt there, visual_projection.weight = proj.T
      * the flat layout itself.
    A file of a whole model (OpenAI's model.state_dict() or ViT-B-16.pt, open_clip's) works too: where any key carries one of the
    prefixes visual.trunk. / vision_model. / visual. / trunk., only the keys under the longest of them are read, so the text tower's
    positional_embedding and transformer.resblocks.* never mix in.  Tensors stored as fp16 are widened.  A missing key raises KeyError
    naming it."""
    family = _family(family)
    where = path if isinstance(path, str) else "state_dict"
    raw = _torch_load(path) if isinstance(path, (str, os.PathLike)) else dict(path)
    # a file of a whole model holds the text tower beside the vision tower, partly under the same names (OpenAI's positional_embedding
    # and transformer.resblocks.N.* exist unprefixed for the text and under visual. for the image): where any key carries a known
    # prefix, ONLY the keys under the longest such prefix are the tower, and unprefixed keys are never mixed in - except transformers'
    # visual_projection.weight, which sits beside vision_model.* by design
    pre = next((p for p in _PREFIXES if any(k.startswith(p) for k in raw)), None)
    if pre is None:
        sd = dict(raw)
    else:
        sd = {k[len(pre):]: v for k, v in raw.items() if k.startswith(pre)}
        if pre == "vision_model." and "visual_projection.weight" in raw:
            sd["visual_projection.weight"] = raw["visual_projection.weight"]

    def get(k):
        if k not in sd:
            raise KeyError(f"{k} not in {where}")
        return sd[k].detach().to(torch.float32)

    def depth_of(pattern):
        return 1 + max((int(m.group(1)) for m in (re.match(pattern, k) for k in sd) if m), default=-1)

    out: Dict[str, torch.Tensor] = {}

    def copy_wb(dst, src):
        out[f"{dst}.weight"], out[f"{dst}.bias"] = get(f"{src}.weight").clone(), get(f"{src}.bias").clone()

    def hf_blocks():
        depth = depth_of(r"encoder\.layers\.(\d+)\.")
        for i in range(depth):
            b = f"encoder.layers.{i}"
            out[f"blocks.{i}.qkv.weight"] = torch.cat([get(f"{b}.self_attn.{x}_proj.weight") for x in "qkv"])
            out[f"blocks.{i}.qkv.bias"] = torch.cat([get(f"{b}.self_attn.{x}_proj.bias") for x in "qkv"])
            for leaf, src in _HF_BLOCK.items():
                copy_wb(f"blocks.{i}.{leaf}", f"{b}.{src}")
        return depth

    if "patch.weight" in sd:                                                   # the flat layout
        depth = depth_of(r"blocks\.(\d+)\.")
        for k in _flat_keys(family, depth):
            out[k] = get(k).clone()
        for k in ("heads", "image_size"):
            if k in sd:
                out[k] = torch.as_tensor(sd[k]).to(torch.int64).reshape(())
    elif family == "siglip" and "patch_embed.proj.weight" in sd:               # timm
        copy_wb("patch", "patch_embed.proj")
        out["pos"] = get("pos_embed").reshape(-1, out["patch.weight"].shape[0]).clone()
        depth = depth_of(r"blocks\.(\d+)\.")
        for i in range(depth):
            for leaf, src in _TIMM_BLOCK.items():
                copy_wb(f"blocks.{i}.{leaf}", f"blocks.{i}.{src}")
        copy_wb("ln_post", "norm")
        out["pool.probe"] = get("attn_pool.latent").reshape(-1).clone()
        for leaf, src in (("q", "q"), ("kv", "kv"), ("proj", "proj"), ("ln", "norm"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            copy_wb(f"pool.{leaf}", f"attn_pool.{src}")
    elif family == "siglip":                                                   # transformers
        copy_wb("patch", "embeddings.patch_embedding")
        out["pos"] = get("embeddings.position_embedding.weight").clone()
        depth = hf_blocks()
        copy_wb("ln_post", "post_layernorm")
        out["pool.probe"] = get("head.probe").reshape(-1).clone()
        w, b, c = get("head.attention.in_proj_weight"), get("head.attention.in_proj_bias"), out["patch.weight"].shape[0]
        out["pool.q.weight"], out["pool.q.bias"] = w[:c].clone(), b[:c].clone()
        out["pool.kv.weight"], out["pool.kv.bias"] = w[c:].clone(), b[c:].clone()
        for leaf, src in (("proj", "attention.out_proj"), ("ln", "layernorm"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            copy_wb(f"pool.{leaf}", f"head.{src}")
    elif "conv1.weight" in sd:                                                 # OpenAI
        out["patch.weight"] = get("conv1.weight").clone()
        out["cls"], out["pos"], out["proj"] = get("class_embedding").clone(), get("positional_embedding").clone(), get("proj").clone()
        copy_wb("ln_pre", "ln_pre")
        depth = depth_of(r"transformer\.resblocks\.(\d+)\.")
        for i in range(depth):
            b = f"transformer.resblocks.{i}"
            out[f"blocks.{i}.qkv.weight"], out[f"blocks.{i}.qkv.bias"] = get(f"{b}.attn.in_proj_weight").clone(), get(f"{b}.attn.in_proj_bias").clone()
            for leaf, src in _OPENAI_BLOCK.items():
                copy_wb(f"blocks.{i}.{leaf}", f"{b}.{src}")
        copy_wb("ln_post", "ln_post")
    else:                                                                      # transformers
        out["patch.weight"] = get("embeddings.patch_embedding.weight").clone()
        out["cls"], out["pos"] = get("embeddings.class_embedding").clone(), get("embeddings.position_embedding.weight").clone()
        copy_wb("ln_pre", "pre_layrnorm")
        depth = hf_blocks()
        copy_wb("ln_post", "post_layernorm")
        out["proj"] = get("visual_projection.weight").t().contiguous()
    if depth < 1:
        raise KeyError(f"blocks.0.ln1.weight (no transformer block) not in {where}")
    if "heads" not in out:
        out["heads"] = torch.tensor(_default_heads(out["patch.weight"].shape[0]))
    if "image_size" not in out:
        ncls = 0 if family == "siglip" else 1
        out["image_size"] = torch.tensor(_default_image_size(family, out["patch.weight"].shape[-1], int(round((out["pos"].shape[0] - ncls) ** 0.5))))
    vit_config_from_state(out)                                                 # shapes make a tower
    return out


# ---------------------------------------------------------------- the definition, on the CPU
def nearest_index_table(n_in: int, n_out: int) -> torch.Tensor:
    """int64 [n_out]: the source index F.interpolate(mode='nearest') reads for every destination index along an axis of n_in ->
    n_out samples, obtained by running F.interpolate itself over an index ramp (exact in float32 below 2^24): no restatement of its
    rounding rule anywhere in this package.  The 2-D resize is the outer product of two such tables."""
    assert 0 < n_in < 2 ** 24 and n_out > 0
    ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in)
    return F.interpolate(ramp, size=n_out, mode="nearest").view(n_out).to(torch.int64)


def _norm_constants(family: str, dtype):
    mean = torch.tensor(CLIP_MEAN[family], dtype=torch.float32).to(dtype)      # float32 values on both sides
    std = torch.tensor(CLIP_STD[family], dtype=torch.float32).to(dtype)
    return mean, std


def clip_resized_input(img_u8, size: int, family: str, bgr: bool = True, normalize: bool = False, dtype=torch.float64) -> torch.Tensor:
    """uint8 [N, H, W, 3] RGB -> what the tower is fed, NCHW [N, 3, size, size].  In float32 this is the operation order of
    ssr_vit_patch_input: / 255, then (x - mean) / std."""
    x = torch.as_tensor(img_u8)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3, "uint8 [N, H, W, 3]"
    x = x.cpu()
    rows, cols = nearest_index_table(x.shape[1], size), nearest_index_table(x.shape[2], size)
    x = x[:, rows][:, :, cols].to(dtype) / 255
    if bgr:
        x = x.flip(-1)
    if normalize:
        mean, std = _norm_constants(family, dtype)
        x = (x - mean) / std
    return x.permute(0, 3, 1, 2).contiguous()


def _act(x, family: str, gelu: str):
    if family == "clip":
        return x * torch.sigmoid(1.702 * x)
    return F.gelu(x, approximate="tanh" if gelu == "tanh" else "none")


def _attention(q, k, v, heads: int):
    """q [N, Tq, C], k, v [N, Tk, C] -> [N, Tq, C]"""
    n, tq, c = q.shape
    d = c // heads
    sp = lambda t: t.reshape(n, t.shape[1], heads, d).transpose(1, 2)          # noqa: E731
    a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * d ** -0.5, dim=-1) @ sp(v)
    return a.transpose(1, 2).reshape(n, tq, c)


def vit_features_from_input(x: torch.Tensor, state: Dict[str, torch.Tensor], gelu: str = "tanh", tower_arithmetic: str = "exact") -> torch.Tensor:
    """the tower on an NCHW input in the input's dtype -> [N, out_dim].  tower_arithmetic 'split': every matrix product is
    linear_split.linear_split_reference with fp16 pieces (the patch embedding as a product over the patch matrix)."""
    cfg = vit_config_from_state(state)
    fam, heads, eps, dt = cfg["family"], cfg["heads"], cfg["ln_eps"], x.dtype
    W = lambda k: state[k].to(dt)                                              # noqa: E731
    mm = F.linear
    if check_tower_arithmetic(tower_arithmetic, "tower_arithmetic") == "split":
        mm = lambda t, w, b=None: linear_split_reference(t, w, b, "f16").to(dt)  # noqa: E731
    lin = lambda t, name: mm(t, W(f"{name}.weight"), W(f"{name}.bias"))        # noqa: E731
    ln = lambda t, name: F.layer_norm(t, (cfg["width"],), W(f"{name}.weight"), W(f"{name}.bias"), eps)       # noqa: E731
    if mm is F.linear:
        x = F.conv2d(x, W("patch.weight"), W("patch.bias") if fam == "siglip" else None, stride=cfg["patch"]).flatten(2).transpose(1, 2)
    else:
        n, p, g = x.shape[0], cfg["patch"], cfg["grid"]
        patches = x[:, :, :g * p, :g * p].reshape(n, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * p * p)
        x = mm(patches, W("patch.weight").reshape(cfg["width"], -1), W("patch.bias") if fam == "siglip" else None)
    if fam == "clip":
        x = torch.cat([W("cls").expand(x.shape[0], 1, -1), x], dim=1)
    x = x + W("pos")
    if fam == "clip":
        x = ln(x, "ln_pre")
    for i in range(cfg["depth"]):
        b = f"blocks.{i}"
        q, k, v = lin(ln(x, f"{b}.ln1"), f"{b}.qkv").chunk(3, dim=-1)
        x = x + lin(_attention(q, k, v, heads), f"{b}.proj")
        x = x + lin(_act(lin(ln(x, f"{b}.ln2"), f"{b}.fc1"), fam, gelu), f"{b}.fc2")
    if fam == "clip":
        return ln(x[:, 0], "ln_post") @ W("proj") if mm is F.linear else mm(ln(x[:, 0], "ln_post"), W("proj").t())
    x = ln(x, "ln_post")
    q = lin(W("pool.probe").expand(x.shape[0], 1, -1), "pool.q")
    k, v = lin(x, "pool.kv").chunk(2, dim=-1)
    a = lin(_attention(q, k, v, heads), "pool.proj")
    a = a + lin(_act(lin(ln(a, "pool.ln"), "pool.fc1"), fam, gelu), "pool.fc2")
    return a[:, 0]


def clip_image_features_reference(state: Dict[str, torch.Tensor], images_u8, bgr: bool = True, normalize: bool = False, gelu: str = "tanh",
                                  dtype=torch.float64, tower_arithmetic: str = "exact") -> torch.Tensor:
    """model.encode_image of uint8 [N, H, W, 3] RGB images as the reference feeds them (module docstring) -> [N, out_dim]"""
    cfg = vit_config_from_state(state)
    with torch.no_grad():
        return vit_features_from_input(clip_resized_input(images_u8, cfg["image_size"], cfg["family"], bgr, normalize, dtype), state, gelu,
                                       tower_arithmetic)


def cosine_pairs_reference(fa: torch.Tensor, fb: torch.Tensor) -> torch.Tensor:
    fa, fb = fa.double(), fb.double()
    return (fa * fb).sum(-1) / (fa.pow(2).sum(-1).sqrt() * fb.pow(2).sum(-1).sqrt()).clamp_min(COS_EPS)


def clipscore_reference(a_u8, b_u8, state: Dict[str, torch.Tensor], bgr: bool = True, normalize: bool = False, gelu: str = "tanh",
                        dtype=torch.float64) -> torch.Tensor:
    """CLIPScore of uint8 [N, H, W, 3] RGB image pairs -> float64 [N]"""
    return cosine_pairs_reference(clip_image_features_reference(state, a_u8, bgr, normalize, gelu, dtype),
                                  clip_image_features_reference(state, b_u8, bgr, normalize, gelu, dtype))


# ---------------------------------------------------------------- the device path
class CLIPVisualModel(TowerWeights):
    """The weights of one tower of either family (vit_tower.TowerWeights, no backward) and the plans that use them, cached per
    (B, H, W, bgr, normalize, tower_attention)."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda", gelu: str = "tanh", tower_arithmetic: str = "exact",
                 tower_attention: str = "fma"):
        if gelu not in _GELUS:
            raise NotImplementedError(f"gelu={gelu!r} (have {list(_GELUS)})")
        super().__init__(state, device, gelu, check_tower_arithmetic(tower_arithmetic, "metric type 'calculate_clipscore': tower_arithmetic"),
                         check_tower_attention(tower_attention, "metric type 'calculate_clipscore': tower_attention"),
                         "metric type 'calculate_clipscore'")
        self.plans: Dict[Tuple, CLIPVisualPlan] = {}

    def plan(self, B: int, H: int, W: int, bgr: bool = True, normalize: bool = False) -> "CLIPVisualPlan":
        key = (B, H, W, bool(bgr), bool(normalize), self.tower_attention)
        if key not in self.plans:
            self.plans[key] = CLIPVisualPlan(self, B, H, W, bgr, normalize)
        return self.plans[key]


class CLIPVisualPlan(TowerPlan):
    """One static launch list for B uint8 images of H x W: ssr_vit_patch_input (resize, channel order, / 255, mean / std), then one
    pass of vit_tower.TowerPlan.forward with the rows updated in place and the activation fused into fc1.  `features` [B, out_dim]
    stays on the device; `run_pairs()` appends ssr_cosine_pairs for B = 2 N."""

    def __init__(self, model: CLIPVisualModel, B: int, H: int, W: int, bgr: bool = True, normalize: bool = False):
        from . import engine, hip
        super().__init__(model, B, H, W, "CLIPScore")
        fam, Cw, p, g, T, mlp, E, depth = (model.cfg[k] for k in ("family", "width", "patch", "grid", "tokens", "mlp", "out_dim", "depth"))
        G, M = g * g, B * T
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=model.device)      # noqa: E731
        self.u8 = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=model.device)
        self._perm = (C.c_int32 * 3)(*((2, 1, 0) if bgr else (0, 1, 2)))
        self._mean, self._std = ((C.c_float * 3)(*t[fam]) if normalize else None for t in (CLIP_MEAN, CLIP_STD))
        b = self.bufs = {"patches": z(B * G, 3 * p * p), "embed": z(B * G, Cw), "x": z(M, Cw), "h": z(M, Cw), "qkv": z(M, 3 * Cw), "att": z(M, Cw),
                         "post": z(M, mlp), "features": z(B, E)}
        if fam == "clip":
            b["pooled"] = z(B, Cw)
        else:
            b.update(probe=model.w["pool.probe"].reshape(1, Cw).repeat(B, 1).contiguous(), q=z(B, Cw), kv=z(M, 2 * Cw), pa=z(B, Cw), py=z(B, Cw),
                     pz=z(B, Cw), pm=z(B, mlp))

        def patch_input(L, patches):
            L.add(self.lib.ssr_vit_patch_input, self.u8.data_ptr(), B, H, W, self.rowidx.data_ptr(), self.colidx.data_ptr(), g, p, patches,
                  hip.F32, self._perm, self._mean, self._std, what="patch input")

        self.launcher = engine.Launcher()
        self.forward(self.launcher, patch_input, b, [b["x"]] * (depth + 1), [b["qkv"]] * depth, [b["x"]] * depth, None,
                     None if fam == "clip" else (b["q"], b["kv"], b["py"], None), b["features"])
        self.features = b["features"]
        self.scores = None

    def run(self, images_u8: torch.Tensor) -> torch.Tensor:
        """-> the features [B, out_dim], fp32, on the device (the plan's own buffer: overwritten by the next run)"""
        self.u8.copy_(images_u8)
        self.launcher.run()
        return self.features

    def run_pairs(self, a_u8: torch.Tensor, b_u8: torch.Tensor) -> torch.Tensor:
        """B = 2 N: images a then images b in ONE pass -> float64 [N] on the host"""
        from . import hip
        N = self.B // 2
        assert self.B == 2 * N and a_u8.shape[0] == N
        if self.scores is None:
            self.scores = torch.zeros(N, dtype=torch.float64, device=self.model.device)
        self.u8[:N].copy_(a_u8)
        self.u8[N:].copy_(b_u8)
        self.launcher.run()
        hip.check(hip.lib().ssr_cosine_pairs(hip.view(self.features), hip.F32, N, self.features.shape[1], self.scores.data_ptr(),
                                             hip.stream_ptr()), "ssr_cosine_pairs")
        return self.scores.cpu()


def clip_image_features(images_u8: torch.Tensor, model: CLIPVisualModel, bgr: bool = True, normalize: bool = False) -> torch.Tensor:
    """uint8 [B, H, W, 3] RGB device images -> a copy of the features, fp32 [B, out_dim] on the device"""
    if images_u8.dtype != torch.uint8 or not images_u8.is_cuda or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError(f"CLIPScore needs uint8 [N, H, W, 3] device images, got {tuple(images_u8.shape)} {images_u8.dtype}")
    n, h, w, _ = images_u8.shape
    return model.plan(n, h, w, bgr, normalize).run(images_u8.contiguous()).clone()


def clipscore(a_u8: torch.Tensor, b_u8: torch.Tensor, model: CLIPVisualModel, bgr: bool = True, normalize: bool = False) -> torch.Tensor:
    """a_u8, b_u8: uint8 [N, H, W, 3] RGB device tensors as `tensor2img_u8` gives them -> float64 [N] on the host.  Both images of
    every pair go through the tower in one pass (a batch of 2 N)."""
    if not (a_u8.shape == b_u8.shape and a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.is_cuda and b_u8.is_cuda):
        raise ValueError(f"Image shapes are different: {tuple(a_u8.shape)}, {tuple(b_u8.shape)} (uint8 device tensors)")
    if a_u8.dim() != 4 or a_u8.shape[-1] != 3:
        raise ValueError(f"CLIPScore needs uint8 [N, H, W, 3] images, got {tuple(a_u8.shape)}")
    n, h, w, _ = a_u8.shape
    return model.plan(2 * n, h, w, bgr, normalize).run_pairs(a_u8.contiguous(), b_u8.contiguous())


# ---------------------------------------------------------------- the metric entry
_MODELS: Dict[Tuple, CLIPVisualModel] = {}


def _model_key(family: str, path: str, device_index, gelu: str, tower_arithmetic: str, tower_attention: str) -> Tuple:
    """what one cached tower (and so its plans) is loaded per"""
    return (family, path, device_index, gelu, tower_arithmetic, tower_attention)
_SAVE_HINT = {
    "siglip": "torch.save(open_clip.create_model_and_transforms('ViT-SO400M-14-SigLIP-384', pretrained='webli')[0].visual.state_dict(), <file>)",
    "clip": "torch.save(clip.load('ViT-B/16', device='cpu')[0].state_dict(), <file>), or the downloaded ViT-B-16.pt itself",
}


def check_clipscore_opt(clip_model=None, **kw) -> Tuple[str, str, str]:
    """Validates the keys of a `calculate_clipscore` entry and finds the weights -> (family, weights file, gelu).  Touches no
    device: the model plugin calls it before the first validation image is processed."""
    if clip_model in CLIP_REFUSED:
        raise NotImplementedError(f"metric type 'calculate_clipscore': clip_model={clip_model!r} (ViT-bigG-14 CLIPA, 1.8 B parameters) is outside "
                                  f"the MI355X path (have {sorted(CLIP_MODELS)})")
    if clip_model not in CLIP_MODELS:
        raise NotImplementedError(f"metric type 'calculate_clipscore': clip_model={clip_model!r} is not supported for CLIPScore: the reference "
                                  f"offers {sorted(CLIP_MODELS) + list(CLIP_REFUSED)}")
    family = CLIP_MODELS[clip_model]
    for k in kw:
        if k not in _IGNORED_KEYS and k not in _OUR_KEYS:
            raise NotImplementedError(f"metric type 'calculate_clipscore': option {k!r} (have {sorted(_OUR_KEYS + ('clip_model',))})")
    gelu = kw.get("gelu", "tanh")
    if gelu not in _GELUS:
        raise NotImplementedError(f"metric type 'calculate_clipscore': gelu={gelu!r} (have {list(_GELUS)})")
    check_tower_arithmetic(kw.get("tower_arithmetic"), "metric type 'calculate_clipscore': tower_arithmetic")
    check_tower_attention(kw.get("tower_attention"), "metric type 'calculate_clipscore': tower_attention")
    given = kw.get("clip_weights")
    if given:
        if not os.path.exists(given):
            raise FileNotFoundError(f"metric type 'calculate_clipscore': clip_weights={given!r} does not exist")
        return family, os.path.abspath(given), gelu
    env, default = CLIP_ENV[family], CLIP_PRETRAIN_PATH[family]
    for cand in (os.environ.get(env), default):
        if cand and os.path.exists(cand):
            return family, os.path.abspath(cand), gelu
    raise NotImplementedError(
        f"metric type 'calculate_clipscore': no weights found for clip_model={clip_model!r}.  Put them in one of three places: the "
        f"metric's option `clip_weights: <file>`, the environment variable {env}=<file>, or {default}.  Save the file with "
        f"{_SAVE_HINT[family]}.  There is no silent random network: a metric from random weights is not CLIPScore")


def calculate_clipscore(img, img2, clip_model=None, **kw) -> float:
    """One image pair per call (uint8 [1, H, W, 3] or [H, W, 3] RGB on the device), as the other entries of metrics.METRICS; both
    images go through the tower in one pass.  Keys: clip_model ('siglip-ViT-SO400M-14' | 'clip-ViT-B/16'); ours: clip_weights, rgb
    (default false: the reference's BGR feed), normalize (default false: the reference's raw [0, 1] feed), gelu ('tanh' | 'erf',
    siglip only), tower_arithmetic ('exact', the default: ssr_linear | 'split': ssr_linear_split with fp16 pieces), tower_attention
    ('fma', the default: ssr_mha_fwd | 'mfma': ssr_mha_mfma_fwd for the blocks' self-attention).  The loaded tower and its plans are
    cached per (family, resolved path, device, gelu, tower_arithmetic, tower_attention): the reference reloads the model for every image."""
    family, path, gelu = check_clipscore_opt(clip_model, **kw)
    arith = check_tower_arithmetic(kw.get("tower_arithmetic"), "metric type 'calculate_clipscore': tower_arithmetic")
    attn = check_tower_attention(kw.get("tower_attention"), "metric type 'calculate_clipscore': tower_attention")
    a, b = (t if t.dim() == 4 else t[None] for t in (img, img2))
    if a.shape[0] != 1:
        raise ValueError("one image per call (the reference validates with batch size 1)")
    key = _model_key(family, path, a.device.index, gelu, arith, attn)
    if key not in _MODELS:
        _MODELS[key] = CLIPVisualModel(load_clip_visual_state(path, family), a.device, gelu=gelu, tower_arithmetic=arith, tower_attention=attn)
    s = clipscore(a, b, _MODELS[key], bgr=not kw.get("rgb", False), normalize=bool(kw.get("normalize", False)))
    return float(s[0])
