"""CPU: the CLIPScore metric's definition, loader, index tables and options (satlas_super_resolution_amd/clipscore_metric.py).
The device path is tests/test_gpu_clipscore.py."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import clipscore_fixture as FX
from conftest import GOLDEN
from satlas_super_resolution_amd import clipscore_metric as CM

FEEDS = {"reference": dict(bgr=True, normalize=False), "rgb+normalize": dict(bgr=False, normalize=True)}


# ------------------------------------------------------------------ the definition against the recorded `transformers` values
@pytest.mark.parametrize("feed", list(FEEDS))
@pytest.mark.parametrize("family", ["siglip", "clip"])
def test_reference_reproduces_the_recorded_fixture(family, feed):
    """both sides are float64 and differ only in operation order: 1e-9 max|ref| is a generous bound"""
    gold, sd = FX.load_golden(family), FX.tiny_state(family)
    assert gold["config"] == FX.TINY[family] and gold["seed"] == FX.SEED[family] and torch.equal(gold["images"], FX.fixture_images())
    want = gold["features"][feed]
    got = CM.clip_image_features_reference(sd, gold["images"], dtype=torch.float64, **FEEDS[feed])
    assert got.dtype == torch.float64 and got.shape == want.shape == (3, CM.vit_config_from_state(sd)["out_dim"])
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())
    for (i, j), s in zip(gold["pairs"], gold["scores"][feed]):
        mine = CM.clipscore_reference(gold["images"][i:i + 1], gold["images"][j:j + 1], sd, **FEEDS[feed])
        assert abs(float(mine[0]) - float(s)) <= 1e-9
    assert abs(float(gold["scores"][feed][2]) - 1) <= 1e-12 and float(gold["scores"][feed][0]) < 0.97       # (1, 1) and (noise, ramp)
    # the fixture is neither flat nor saturated: the feeds and the images give different features
    assert float((gold["features"]["reference"] - gold["features"]["rgb+normalize"]).abs().max()) > 0.1
    assert float((want[0] - want[1]).abs().max()) > 0.1


@pytest.mark.parametrize("family", ["siglip", "clip"])
def test_reference_matches_transformers_live(family):
    """the same check against the package's class itself, where it is installed"""
    pytest.importorskip("transformers")
    sd = FX.tiny_state(family)
    cfg = CM.vit_config_from_state(sd)
    model = FX.hf_model(family, sd)
    x = CM.clip_resized_input(FX.fixture_images(), cfg["image_size"], family, dtype=torch.float64)
    want = FX.hf_features(family, model, x)
    got = CM.clip_image_features_reference(sd, FX.fixture_images())
    assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_gelu_option_changes_siglip_only():
    imgs = FX.fixture_images()[:1]
    s, c = FX.tiny_state("siglip"), FX.tiny_state("clip")
    d = (CM.clip_image_features_reference(s, imgs, gelu="tanh") - CM.clip_image_features_reference(s, imgs, gelu="erf")).abs().max()
    assert 1e-6 < float(d) < 1e-1                                            # the two GELUs differ by at most 4.7e-4 per evaluation
    assert torch.equal(CM.clip_image_features_reference(c, imgs, gelu="tanh"), CM.clip_image_features_reference(c, imgs, gelu="erf"))


def test_softmax_of_the_fixture_is_neither_flat_nor_one_hot():
    """the rule's scales: the largest attention probability of a query, averaged, lies in [0.15, 0.9] in the first block"""
    for family in ("siglip", "clip"):
        sd = FX.tiny_state(family)
        cfg = CM.vit_config_from_state(sd)
        x = CM.clip_resized_input(FX.fixture_images(), cfg["image_size"], family)
        t = F.conv2d(x, sd["patch.weight"].double(), sd["patch.bias"].double() if family == "siglip" else None, stride=cfg["patch"]).flatten(2).transpose(1, 2)
        if family == "clip":
            t = torch.cat([sd["cls"].double().expand(3, 1, -1), t], dim=1)
        t = t + sd["pos"].double()
        if family == "clip":
            t = F.layer_norm(t, (cfg["width"],), sd["ln_pre.weight"].double(), sd["ln_pre.bias"].double(), 1e-5)
        h = F.layer_norm(t, (cfg["width"],), sd["blocks.0.ln1.weight"].double(), sd["blocks.0.ln1.bias"].double(), cfg["ln_eps"])
        q, k, _ = F.linear(h, sd["blocks.0.qkv.weight"].double(), sd["blocks.0.qkv.bias"].double()).chunk(3, dim=-1)
        sp = lambda u: u.reshape(3, -1, cfg["heads"], cfg["head_dim"]).transpose(1, 2)        # noqa: E731
        p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * cfg["head_dim"] ** -0.5, dim=-1)
        peak = float(p.max(dim=-1).values.mean())
        assert 0.15 <= peak <= 0.9, (family, peak)


# ------------------------------------------------------------------ the loader
def _same(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def _with_meta(sd, family):
    cfg = CM.vit_config_from_state(sd)
    return dict(sd, image_size=torch.tensor(cfg["image_size"]))


@pytest.mark.parametrize("layout", ["timm", "timm visual.trunk.", "timm trunk.", "hf", "hf vision_model.", "flat"])
def test_loader_siglip_layouts_map_bit_for_bit(layout, tmp_path):
    sd = FX.tiny_state("siglip")
    src = {"timm": lambda: FX.to_timm_siglip(sd), "timm visual.trunk.": lambda: FX.to_timm_siglip(sd, "visual.trunk."),
           "timm trunk.": lambda: FX.to_timm_siglip(sd, "trunk."), "hf": lambda: FX.to_hf_siglip(sd),
           "hf vision_model.": lambda: FX.to_hf_siglip(sd, "vision_model."), "flat": lambda: dict(sd)}[layout]()
    src["logit_scale"], src["logit_bias"] = torch.tensor(1.0), torch.tensor(-10.0)      # keys of the rest of the model are ignored
    if "." in layout:                                                        # a whole open_clip model: the text tower beside the prefixed trunk
        src.update({"text.pos_embed": torch.zeros(1, 64, 32), "text.blocks.0.norm1.weight": torch.zeros(32), "norm.weight": torch.zeros(7)})
    torch.save(src, tmp_path / "w.pth")
    _same(CM.load_clip_visual_state(str(tmp_path / "w.pth"), "siglip"), _with_meta(sd, "siglip"))
    _same(CM.load_clip_visual_state(src, "siglip"), _with_meta(sd, "siglip"))        # an already loaded state_dict


@pytest.mark.parametrize("layout", ["openai visual.", "openai", "openai whole model", "hf", "flat", "state_dict wrapper"])
def test_loader_clip_layouts_map_bit_for_bit(layout, tmp_path):
    sd = FX.tiny_state("clip")
    src = {"openai visual.": lambda: FX.to_openai_clip(sd), "openai": lambda: FX.to_openai_clip(sd, ""), "hf": lambda: FX.to_hf_clip(sd),
           "flat": lambda: dict(sd), "state_dict wrapper": lambda: {"state_dict": FX.to_openai_clip(sd)},
           "openai whole model": lambda: FX.to_openai_clip_whole_model(sd)}[layout]()
    if layout == "openai visual.":
        src["token_embedding.weight"] = torch.zeros(4, 4)                    # the text tower's keys are ignored
    torch.save(src, tmp_path / "w.pt")
    _same(CM.load_clip_visual_state(str(tmp_path / "w.pt"), "clip"), _with_meta(sd, "clip"))


def test_loader_widens_fp16_storage(tmp_path):
    sd = FX.tiny_state("clip")
    half = {k: v.half() for k, v in FX.to_openai_clip(sd).items()}
    torch.save(half, tmp_path / "w.pt")
    got = CM.load_clip_visual_state(str(tmp_path / "w.pt"), "clip")
    for k, v in sd.items():
        if k != "heads":
            assert got[k].dtype == torch.float32 and torch.equal(got[k], v.half().float()), k


@pytest.mark.parametrize("whole", [False, True], ids=["vision tower", "whole model"])
def test_loader_reads_a_torchscript_archive(tmp_path, whole):
    """OpenAI's file is a TorchScript archive: torch.load refuses it and the loader falls back to torch.jit.load.  The whole model
    holds the text tower too: an unprefixed positional_embedding ahead of the visual keys, transformer.resblocks.* of another depth
    and width, text_projection, logit_scale, ln_final - only the keys under visual. are the tower."""
    sd = FX.tiny_state("clip")

    class Holder(torch.nn.Module):
        def forward(self, x):
            return x

    def build(parent, parts, value):
        if len(parts) == 1:
            parent.register_parameter(parts[0], torch.nn.Parameter(value.clone(), requires_grad=False))
            return
        if not hasattr(parent, parts[0]):
            parent.add_module(parts[0], Holder())
        build(getattr(parent, parts[0]), parts[1:], value)

    root = Holder()
    for k, v in (FX.to_openai_clip_whole_model(sd) if whole else FX.to_openai_clip(sd)).items():
        build(root, k.split("."), v)
    if whole:
        assert list(root.state_dict())[0] == "positional_embedding" and "transformer.resblocks.2.ln_1.weight" in root.state_dict()
    path = str(tmp_path / "ViT-tiny.pt")
    torch.jit.script(root).save(path)
    with pytest.raises(Exception):
        torch.load(path, map_location="cpu", weights_only=True)
    _same(CM.load_clip_visual_state(path, "clip"), _with_meta(sd, "clip"))


@pytest.mark.parametrize("family,missing", [("siglip", "visual.trunk.attn_pool.kv.bias"), ("siglip", "visual.trunk.blocks.1.mlp.fc2.weight"),
                                            ("clip", "visual.ln_post.weight"), ("clip", "visual.transformer.resblocks.0.attn.in_proj_bias")])
def test_loader_names_a_missing_key(family, missing):
    sd = FX.tiny_state(family)
    src = FX.to_timm_siglip(sd, "visual.trunk.") if family == "siglip" else FX.to_openai_clip(sd)
    del src[missing]
    with pytest.raises(KeyError, match=missing.split(".", 2 if family == "siglip" else 1)[-1].replace(".", r"\.")):
        CM.load_clip_visual_state(src, family)
    hf = FX.to_hf_siglip(sd) if family == "siglip" else FX.to_hf_clip(sd)
    del hf[[k for k in hf if k.endswith("post_layernorm.bias")][0]]
    with pytest.raises(KeyError, match=r"post_layernorm\.bias"):
        CM.load_clip_visual_state(hf, family)


def test_config_of_real_shape_key_sets():
    """shapes only (meta tensors): no 1.7 GB allocation"""
    m = lambda *s: torch.empty(*s, device="meta")                            # noqa: E731
    so = FX.flat_shapes("siglip", 1152, 27, 4304, 14, 27)
    st = {k: m(*so[k]) for k in CM._flat_keys("siglip", 27)}
    cfg = CM.vit_config_from_state(st)
    assert cfg == {"family": "siglip", "width": 1152, "patch": 14, "depth": 27, "grid": 27, "tokens": 729, "mlp": 4304, "heads": 16, "head_dim": 72,
                   "out_dim": 1152, "image_size": 384, "ln_eps": 1e-6, "class_token": False}
    b16 = FX.flat_shapes("clip", 768, 12, 3072, 16, 14, 512)
    st = {k: m(*b16[k]) for k in CM._flat_keys("clip", 12)}
    cfg = CM.vit_config_from_state(st)
    assert cfg == {"family": "clip", "width": 768, "patch": 16, "depth": 12, "grid": 14, "tokens": 197, "mlp": 3072, "heads": 12, "head_dim": 64,
                   "out_dim": 512, "image_size": 224, "ln_eps": 1e-5, "class_token": True}
    tiny = CM.vit_config_from_state(FX.tiny_state("siglip"))
    assert (tiny["width"], tiny["heads"], tiny["head_dim"], tiny["mlp"], tiny["depth"], tiny["image_size"]) == (144, 2, 72, 200, 2, 42)
    with pytest.raises(KeyError, match="pos"):
        CM.vit_config_from_state({"patch.weight": m(8, 3, 2, 2)})
    with pytest.raises(ValueError, match="grid"):
        CM.vit_config_from_state(dict(st, pos=m(196, 768)))
    with pytest.raises(ValueError, match="image_size"):
        CM.vit_config_from_state(dict(FX.tiny_state("siglip"), image_size=torch.tensor(56)))


def test_random_state_has_the_real_sizes_by_default():
    sd = CM.clip_random_state("clip", depth=1)
    cfg = CM.vit_config_from_state(sd)
    assert (cfg["width"], cfg["mlp"], cfg["patch"], cfg["grid"], cfg["heads"], cfg["out_dim"], cfg["image_size"]) == (768, 3072, 16, 14, 12, 512, 224)
    assert set(sd) == set(CM._flat_keys("clip", 1)) | {"heads", "image_size"}
    t = CM.clip_random_state("siglip", width=144, depth=1, mlp=200, patch=14, grid=3, heads=2)
    f = CM.clip_image_features_reference(t, FX.fixture_images())
    assert f.shape == (3, 144) and bool(torch.isfinite(f).all()) and 0.05 < float(f.abs().max()) < 50


# ------------------------------------------------------------------ the index tables
@pytest.mark.parametrize("H,W,S", [(37, 53, 42), (128, 128, 224), (128, 128, 384), (500, 500, 224)])
def test_index_tables_equal_interpolate(H, W, S):
    """the two tables gather exactly what F.interpolate(., (S, S)) (mode 'nearest', the reference's call) returns"""
    u = torch.randint(0, 256, (2, H, W, 3), generator=torch.Generator().manual_seed(H + W + S), dtype=torch.uint8)
    rows, cols = CM.nearest_index_table(H, S), CM.nearest_index_table(W, S)
    assert rows.dtype == torch.int64 and rows.shape == (S,) and int(rows.min()) >= 0 and int(rows.max()) < H and int(cols.max()) < W
    x = u.permute(0, 3, 1, 2).float() / 255
    want = F.interpolate(x, (S, S))
    assert torch.equal(x[:, :, rows][:, :, :, cols], want)
    got = CM.clip_resized_input(u, S, "clip", bgr=False, normalize=False, dtype=torch.float32)
    assert torch.equal(got, want)


# ------------------------------------------------------------------ options
def test_feed_options_change_the_input_as_documented():
    u = FX.fixture_images()[:1]
    base = CM.clip_resized_input(u, 42, "clip", bgr=False, normalize=False)
    assert torch.equal(CM.clip_resized_input(u, 42, "clip", bgr=True, normalize=False), base.flip(1))                 # the reference's BGR feed
    mean, std = (torch.tensor(v, dtype=torch.float32).double().view(1, 3, 1, 1) for v in (CM.CLIP_MEAN["clip"], CM.CLIP_STD["clip"]))
    assert torch.equal(CM.clip_resized_input(u, 42, "clip", bgr=False, normalize=True), (base - mean) / std)          # OpenAI's constants
    assert torch.equal(CM.clip_resized_input(u, 42, "siglip", bgr=False, normalize=True), (base - 0.5) / 0.5)
    assert float(base.min()) >= 0 and float(base.max()) <= 1 and CM.CLIP_MEAN["clip"] == (0.48145466, 0.4578275, 0.40821073)


def test_options(tmp_path, monkeypatch):
    from satlas_super_resolution_amd import metrics as M
    assert M.METRICS["calculate_clipscore"] is CM.calculate_clipscore and M.METRIC_CHECKS["calculate_clipscore"] is CM.check_clipscore_opt
    for env in CM.CLIP_ENV.values():
        monkeypatch.delenv(env, raising=False)
    monkeypatch.chdir(tmp_path)
    w = tmp_path / "w.pth"
    torch.save(FX.tiny_state("siglip"), w)
    assert CM.check_clipscore_opt(clip_model="siglip-ViT-SO400M-14", clip_weights=str(w)) == ("siglip", str(w.resolve()), "tanh")
    assert CM.check_clipscore_opt(clip_model="clip-ViT-B/16", clip_weights=str(w), gelu="erf", rgb=True, normalize=True, crop_border=4,
                                  test_y_channel=False, input_order="HWC", better="higher") == ("clip", str(w.resolve()), "erf")
    with pytest.raises(NotImplementedError, match="clipa-ViT-bigG-14"):
        CM.check_clipscore_opt(clip_model="clipa-ViT-bigG-14", clip_weights=str(w))
    with pytest.raises(NotImplementedError, match="clip-ViT-L/14"):
        CM.check_clipscore_opt(clip_model="clip-ViT-L/14", clip_weights=str(w))
    with pytest.raises(NotImplementedError, match="None"):
        CM.check_clipscore_opt(clip_weights=str(w))
    with pytest.raises(NotImplementedError, match="'img_size'"):
        CM.check_clipscore_opt(clip_model="clip-ViT-B/16", clip_weights=str(w), img_size=224)
    with pytest.raises(NotImplementedError, match="gelu='fast'"):
        CM.check_clipscore_opt(clip_model="siglip-ViT-SO400M-14", clip_weights=str(w), gelu="fast")
    with pytest.raises(FileNotFoundError, match="nope.pth"):
        CM.check_clipscore_opt(clip_model="clip-ViT-B/16", clip_weights=str(tmp_path / "nope.pth"))
    # nothing found: the three places, by name, and no silent random network
    for name, fam in CM.CLIP_MODELS.items():
        with pytest.raises(NotImplementedError) as e:
            CM.check_clipscore_opt(clip_model=name)
        msg = str(e.value)
        assert "clip_weights" in msg and CM.CLIP_ENV[fam] in msg and CM.CLIP_PRETRAIN_PATH[fam] in msg and "no silent random network" in msg
        assert ("open_clip" if fam == "siglip" else "clip.load") in msg
    # the second and the third place
    monkeypatch.setenv("SSR_CLIP_SIGLIP_WEIGHTS", str(w))
    assert CM.check_clipscore_opt(clip_model="siglip-ViT-SO400M-14")[1] == str(w.resolve())
    monkeypatch.delenv("SSR_CLIP_SIGLIP_WEIGHTS")
    os.makedirs(tmp_path / "experiments" / "pretrained_models")
    torch.save(FX.tiny_state("clip"), tmp_path / CM.CLIP_PRETRAIN_PATH["clip"])
    assert CM.check_clipscore_opt(clip_model="clip-ViT-B/16")[1] == str((tmp_path / CM.CLIP_PRETRAIN_PATH["clip"]).resolve())


def test_shipped_option_file_passes_with_a_weights_file(tmp_path, monkeypatch):
    """esrgan_s2naip_urban.yml's test.metrics block as shipped, with clip_weights pointed at a tiny saved state"""
    from satlas_super_resolution_amd import metrics as M
    monkeypatch.delenv("SSR_CLIP_SIGLIP_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)
    block = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]["test"]["metrics"]
    assert block["clipscore"] == {"type": "calculate_clipscore", "clip_model": "siglip-ViT-SO400M-14"}
    assert all(mo["type"] in M.METRICS for mo in block.values()) and len(block) == 5
    entry = {k: v for k, v in block["clipscore"].items() if k not in ("type", "better")}
    with pytest.raises(NotImplementedError, match="no weights found"):
        M.METRIC_CHECKS["calculate_clipscore"](**entry)
    torch.save(FX.to_timm_siglip(FX.tiny_state("siglip"), "visual.trunk."), tmp_path / "siglip.pth")
    fam, path, gelu = M.METRIC_CHECKS["calculate_clipscore"](clip_weights=str(tmp_path / "siglip.pth"), **entry)
    assert (fam, gelu) == ("siglip", "tanh") and CM.vit_config_from_state(CM.load_clip_visual_state(path, fam))["width"] == 144


def test_unreadable_file_names_both_errors(tmp_path):
    p = tmp_path / "junk.pt"
    p.write_bytes(b"not a checkpoint")
    with pytest.raises(ValueError, match=r"(?s)neither torch\.load \(.*\) nor torch\.jit\.load \("):
        CM.load_clip_visual_state(str(p), "clip")
