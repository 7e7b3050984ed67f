"""Shared by the CLIPScore tests and tools/make_clipscore_golden.py: the rule that fills a vision tower's weights, the converters
from the flat layout to the layouts of the packages' checkpoints, and the loader of tests/golden/clipscore_*_tiny.pt.  (Not a test
module.)

No weight file is committed: a tower of any size is FILLED BY A RULE that is exact in float32 and does not depend on a library version
(the rule of tests/osm_disc_fixture.py):

    tensor number t of the flat layout's keys in clipscore_metric._flat_keys order (n elements):
        k = numpy.random.PCG64(1000 * seed + t).random_raw(n) >> 40,   u = float32(k) * 2^-24,   w = (2 u - 1) * float32(scale) + offset

    scale = QKV_SCALE / sqrt(fan_in) for the packed qkv / pool q / pool kv matrices: with LayerNorm'd inputs the logits q . k / sqrt(d)
    then have a standard deviation of about QKV_SCALE^4 / 9 ~ 1.5 (u is uniform: variance 1 / 3), so the softmax is neither flat nor
    one-hot; W_SCALE / sqrt(fan_in) for every other matrix (unit-variance inputs give outputs of variance 3 / 4: activations stay O(1)
    through 27 layers, the residual stream growing like the square root of the depth); PATCH_SCALE / sqrt(3 p^2) for the patch embedding
    (its inputs are pixels in [0, 1]); 0.1 for biases; LayerNorm weights 1 + 0.2 (2 u - 1); 1 for pos, cls, the probe; proj as a matrix.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QKV_SCALE, W_SCALE, PATCH_SCALE = 1.9, 1.5, 3.0
TINY = {"siglip": dict(width=144, heads=2, mlp=200, depth=2, patch=14, grid=3),
        "clip": dict(width=128, heads=2, mlp=512, depth=2, patch=16, grid=3, out_dim=32)}
SEED = {"siglip": 3, "clip": 4}


def rule_tensor(seed: int, t: int, shape, scale: float, offset: float = 0.0) -> torch.Tensor:
    n = math.prod(shape)
    k = np.random.PCG64(1000 * seed + t).random_raw(n) >> np.uint64(40)
    u = k.astype(np.float32) * np.float32(2.0 ** -24)
    w = (np.float32(2.0) * u - np.float32(1.0)) * np.float32(scale) + np.float32(offset)
    assert w.dtype == np.float32
    return torch.from_numpy(w).reshape(shape)


def flat_shapes(family: str, width: int, depth: int, mlp: int, patch: int, grid: int, out_dim=None):
    ncls = 0 if family == "siglip" else 1
    s = {"patch.weight": (width, 3, patch, patch), "patch.bias": (width,), "cls": (width,), "pos": (grid * grid + ncls, width),
         "proj": (width, out_dim or width), "pool.probe": (width,)}
    for name in ["ln_pre", "ln_post", "pool.ln"] + [f"blocks.{i}.{l}" for i in range(depth) for l in ("ln1", "ln2")]:
        s[f"{name}.weight"] = s[f"{name}.bias"] = (width,)
    mats = {"pool.q": (width, width), "pool.kv": (2 * width, width), "pool.proj": (width, width), "pool.fc1": (mlp, width), "pool.fc2": (width, mlp)}
    for i in range(depth):
        mats.update({f"blocks.{i}.qkv": (3 * width, width), f"blocks.{i}.proj": (width, width), f"blocks.{i}.fc1": (mlp, width),
                     f"blocks.{i}.fc2": (width, mlp)})
    for name, shape in mats.items():
        s[f"{name}.weight"], s[f"{name}.bias"] = shape, shape[:1]
    return s


def rule_state(family: str, seed: int, width: int, depth: int, mlp: int, patch: int, grid: int, heads: int, out_dim=None):
    """the flat layout (clipscore_metric's module docstring) of a tower of these sizes, filled by the rule"""
    from satlas_super_resolution_amd import clipscore_metric as CM
    shapes = flat_shapes(family, width, depth, mlp, patch, grid, out_dim)
    sd = {}
    for t, key in enumerate(CM._flat_keys(family, depth)):
        shape = shapes[key]
        leaf = key.rsplit(".", 1)[0].rsplit(".", 1)[-1]
        if key == "patch.weight":
            sd[key] = rule_tensor(seed, t, shape, PATCH_SCALE / math.sqrt(3 * patch * patch))
        elif key in ("pos", "cls", "pool.probe"):
            sd[key] = rule_tensor(seed, t, shape, 1.0)
        elif key == "proj":
            sd[key] = rule_tensor(seed, t, shape, W_SCALE / math.sqrt(shape[0]))
        elif leaf.startswith("ln") and key.endswith(".weight"):
            sd[key] = rule_tensor(seed, t, shape, 0.2, 1.0)
        elif key.endswith(".bias"):
            sd[key] = rule_tensor(seed, t, shape, 0.1)
        else:
            s = QKV_SCALE if leaf in ("qkv", "q", "kv") else W_SCALE
            sd[key] = rule_tensor(seed, t, shape, s / math.sqrt(shape[1]))
    sd["heads"] = torch.tensor(heads)
    return sd


def tiny_state(family: str):
    return rule_state(family, SEED[family], **TINY[family])


# ------------------------------------------------------------------ the flat layout written out in the packages' layouts
_HF_BLOCK = {"ln1": "layer_norm1", "proj": "self_attn.out_proj", "ln2": "layer_norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
_TIMM_BLOCK = {"ln1": "norm1", "qkv": "attn.qkv", "proj": "attn.proj", "ln2": "norm2", "fc1": "mlp.fc1", "fc2": "mlp.fc2"}
_OPENAI_BLOCK = {"ln1": "ln_1", "proj": "attn.out_proj", "ln2": "ln_2", "fc1": "mlp.c_fc", "fc2": "mlp.c_proj"}


def _depth(sd):
    return 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))


def _wb(out, dst, sd, src):
    out[f"{dst}.weight"], out[f"{dst}.bias"] = sd[f"{src}.weight"], sd[f"{src}.bias"]


def _hf_blocks(out, sd, pre):
    c = sd["patch.weight"].shape[0]
    for i in range(_depth(sd)):
        for j, x in enumerate("qkv"):
            out[f"{pre}encoder.layers.{i}.self_attn.{x}_proj.weight"] = sd[f"blocks.{i}.qkv.weight"][j * c:(j + 1) * c]
            out[f"{pre}encoder.layers.{i}.self_attn.{x}_proj.bias"] = sd[f"blocks.{i}.qkv.bias"][j * c:(j + 1) * c]
        for leaf, dst in _HF_BLOCK.items():
            _wb(out, f"{pre}encoder.layers.{i}.{dst}", sd, f"blocks.{i}.{leaf}")


def to_hf_siglip(sd, prefix=""):
    """transformers' SiglipVisionModel.state_dict() (prefix 'vision_model.' in older versions of the package)"""
    out, c = {}, sd["patch.weight"].shape[0]
    _wb(out, f"{prefix}embeddings.patch_embedding", sd, "patch")
    out[f"{prefix}embeddings.position_embedding.weight"] = sd["pos"]
    _hf_blocks(out, sd, prefix)
    _wb(out, f"{prefix}post_layernorm", sd, "ln_post")
    out[f"{prefix}head.probe"] = sd["pool.probe"].reshape(1, 1, c)
    out[f"{prefix}head.attention.in_proj_weight"] = torch.cat([sd["pool.q.weight"], sd["pool.kv.weight"]])
    out[f"{prefix}head.attention.in_proj_bias"] = torch.cat([sd["pool.q.bias"], sd["pool.kv.bias"]])
    for leaf, dst in (("proj", "attention.out_proj"), ("ln", "layernorm"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
        _wb(out, f"{prefix}head.{dst}", sd, f"pool.{leaf}")
    return out


def to_timm_siglip(sd, prefix=""):
    """open_clip's model.visual.trunk (a timm VisionTransformer with global_pool='map'); prefix 'visual.trunk.' for the whole model"""
    out, c = {}, sd["patch.weight"].shape[0]
    _wb(out, f"{prefix}patch_embed.proj", sd, "patch")
    out[f"{prefix}pos_embed"] = sd["pos"].reshape(1, -1, c)
    for i in range(_depth(sd)):
        for leaf, dst in _TIMM_BLOCK.items():
            _wb(out, f"{prefix}blocks.{i}.{dst}", sd, f"blocks.{i}.{leaf}")
    _wb(out, f"{prefix}norm", sd, "ln_post")
    out[f"{prefix}attn_pool.latent"] = sd["pool.probe"].reshape(1, 1, c)
    for leaf, dst in (("q", "q"), ("kv", "kv"), ("proj", "proj"), ("ln", "norm"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
        _wb(out, f"{prefix}attn_pool.{dst}", sd, f"pool.{leaf}")
    return out


def to_hf_clip(sd):
    """transformers' CLIPVisionModelWithProjection.state_dict()"""
    out, pre = {}, "vision_model."
    out[f"{pre}embeddings.class_embedding"] = sd["cls"]
    out[f"{pre}embeddings.patch_embedding.weight"] = sd["patch.weight"]
    out[f"{pre}embeddings.position_embedding.weight"] = sd["pos"]
    _wb(out, f"{pre}pre_layrnorm", sd, "ln_pre")
    _hf_blocks(out, sd, pre)
    _wb(out, f"{pre}post_layernorm", sd, "ln_post")
    out["visual_projection.weight"] = sd["proj"].t().contiguous()
    return out


def to_openai_clip(sd, prefix="visual."):
    """OpenAI's CLIP: model.state_dict() restricted to the vision tower"""
    out = {f"{prefix}conv1.weight": sd["patch.weight"], f"{prefix}class_embedding": sd["cls"], f"{prefix}positional_embedding": sd["pos"],
           f"{prefix}proj": sd["proj"]}
    _wb(out, f"{prefix}ln_pre", sd, "ln_pre")
    for i in range(_depth(sd)):
        b = f"{prefix}transformer.resblocks.{i}"
        out[f"{b}.attn.in_proj_weight"], out[f"{b}.attn.in_proj_bias"] = sd[f"blocks.{i}.qkv.weight"], sd[f"blocks.{i}.qkv.bias"]
        for leaf, dst in _OPENAI_BLOCK.items():
            _wb(out, f"{b}.{dst}", sd, f"blocks.{i}.{leaf}")
    _wb(out, f"{prefix}ln_post", sd, "ln_post")
    return out


def to_openai_clip_whole_model(sd, text_width=64, text_depth=3):
    """OpenAI's CLIP: the WHOLE model's state_dict() in its order - the text tower's unprefixed positional_embedding [77, w],
    text_projection and logit_scale, the vision tower under visual., then the text tower's transformer.resblocks.N.* (same leaf names
    as the vision tower's, another depth and width), token_embedding and ln_final"""
    from collections import OrderedDict
    g = torch.Generator().manual_seed(99)
    r = lambda *s: torch.randn(*s, generator=g)                              # noqa: E731
    w = text_width
    out = OrderedDict([("positional_embedding", r(77, w)), ("text_projection", r(w, sd["proj"].shape[1])), ("logit_scale", torch.tensor(4.6))])
    out.update(to_openai_clip(sd, "visual."))
    for i in range(text_depth):
        b = f"transformer.resblocks.{i}"
        out.update({f"{b}.attn.in_proj_weight": r(3 * w, w), f"{b}.attn.in_proj_bias": r(3 * w), f"{b}.attn.out_proj.weight": r(w, w),
                    f"{b}.attn.out_proj.bias": r(w), f"{b}.ln_1.weight": r(w), f"{b}.ln_1.bias": r(w), f"{b}.mlp.c_fc.weight": r(4 * w, w),
                    f"{b}.mlp.c_fc.bias": r(4 * w), f"{b}.mlp.c_proj.weight": r(w, 4 * w), f"{b}.mlp.c_proj.bias": r(w),
                    f"{b}.ln_2.weight": r(w), f"{b}.ln_2.bias": r(w)})
    out.update({"token_embedding.weight": r(50, w), "ln_final.weight": r(w), "ln_final.bias": r(w)})
    return out


# ------------------------------------------------------------------ the `transformers` classes at a flat state's sizes
def hf_model(family: str, sd):
    """the package's class built from a config (random weights), loaded with the flat state, float64, eval"""
    import transformers as T
    from satlas_super_resolution_amd import clipscore_metric as CM
    cfg = CM.vit_config_from_state(sd)
    kw = dict(hidden_size=cfg["width"], intermediate_size=cfg["mlp"], num_hidden_layers=cfg["depth"], num_attention_heads=cfg["heads"],
              image_size=cfg["image_size"], patch_size=cfg["patch"], layer_norm_eps=cfg["ln_eps"], attention_dropout=0.0)
    if family == "siglip":
        m = T.SiglipVisionModel(T.SiglipVisionConfig(hidden_act="gelu_pytorch_tanh", **kw))
        want = to_hf_siglip(sd, "vision_model." if any(k.startswith("vision_model.") for k in m.state_dict()) else "")
    else:
        m = T.CLIPVisionModelWithProjection(T.CLIPVisionConfig(hidden_act="quick_gelu", projection_dim=cfg["out_dim"], **kw))
        want = to_hf_clip(sd)
    m.load_state_dict(want, strict=True)
    return m.double().eval()


def hf_features(family: str, model, x64: torch.Tensor) -> torch.Tensor:
    with torch.no_grad():
        o = model(pixel_values=x64)
    return o.pooler_output if family == "siglip" else o.image_embeds


def fixture_images():
    """uint8 [3, 37, 53, 3]: noise, a smooth ramp with noise, and a near copy of the first (a pair with a score close to 1)"""
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (37, 53, 3), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(37), torch.arange(53), indexing="ij")
    ramp = torch.stack([4 * yy + xx, 3 * xx, 250 - 5 * yy], dim=-1) + torch.randint(0, 24, (37, 53, 3), generator=g)
    c = (a.int() + torch.randint(-8, 9, (37, 53, 3), generator=g, dtype=torch.int32)).clamp(0, 255)
    return torch.stack([a, ramp.clamp(0, 255).to(torch.uint8), c.to(torch.uint8)])


def load_golden(family: str):
    return torch.load(os.path.join(GOLDEN, f"clipscore_{family}_tiny.pt"), weights_only=False)
