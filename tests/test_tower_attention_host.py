"""Host: the option `tower_attention: fma | mfma` of train.clip_opt and of calculate_clipscore (csrc/mha_mfma.hip: the blocks'
self-attention on the fp32-input matrix core) - its values and refusals, that it is orthogonal to tower_arithmetic, what it leaves in
StepConfig.clip, the cache keys, and that the source, the header and hip.py carry the three new entries.  Nothing here needs a device."""
import itertools
import os
import re

import pytest

from conftest import ROOT

WHERES = ("train.clip_opt.tower_attention", "metric type 'calculate_clipscore': tower_attention")
ENTRIES = ("ssr_mha_mfma_fwd", "ssr_mha_mfma_bwd_ws_floats", "ssr_mha_mfma_bwd")


@pytest.mark.parametrize("where", WHERES)
def test_check_tower_attention_values(where):
    from satlas_super_resolution_amd.linear_split import TOWER_ATTENTIONS, check_tower_attention
    assert TOWER_ATTENTIONS == ("fma", "mfma")
    assert check_tower_attention(None, where) == "fma" and check_tower_attention("fma", where) == "fma"
    assert check_tower_attention("mfma", where) == "mfma"
    for bad in ("MFMA", "split", "", 1, True):
        with pytest.raises(NotImplementedError) as e:
            check_tower_attention(bad, where)
        assert str(e.value).startswith(f"{where}={bad!r}") and "'fma'" in str(e.value) and "'mfma'" in str(e.value)


def _clip_block(tmp_path):
    wfile = tmp_path / "w.pth"
    wfile.write_bytes(b"")
    return {"type": "CLIPLoss", "clip_loss_model": "ViT-B-16-SigLIP-256", "clip_weights": str(wfile)}


def test_clip_opt_carries_the_key_only_when_it_is_mfma(tmp_path):
    from satlas_super_resolution_amd import clip_loss as CL
    base = _clip_block(tmp_path)
    assert "tower_attention" in CL._CLIP_OPT_KEYS
    absent = CL.check_clip_opt(dict(base))
    assert "tower_attention" not in absent
    assert CL.check_clip_opt(dict(base, tower_attention="fma")) == absent
    assert CL.check_clip_opt(dict(base, tower_attention="mfma")) == dict(absent, tower_attention="mfma")
    for bad in ("matrix", "Mfma", ""):
        with pytest.raises(NotImplementedError) as e:
            CL.check_clip_opt(dict(base, tower_attention=bad))
        assert str(e.value).startswith(f"train.clip_opt.tower_attention={bad!r}")


def test_clip_opt_reaches_the_step_config(tmp_path):
    import json

    from conftest import GOLDEN
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["cliploss_esrgan_s2naip_urban.yml"]
    opt["train"]["clip_opt"]["clip_weights"] = _clip_block(tmp_path)["clip_weights"]
    assert "tower_attention" not in train_config_from_opt(json.loads(json.dumps(opt))).clip
    opt["train"]["clip_opt"]["tower_attention"] = "fma"
    assert "tower_attention" not in train_config_from_opt(json.loads(json.dumps(opt))).clip
    opt["train"]["clip_opt"]["tower_attention"] = "mfma"
    assert train_config_from_opt(json.loads(json.dumps(opt))).clip["tower_attention"] == "mfma"
    opt["train"]["clip_opt"]["tower_attention"] = "wmma"
    with pytest.raises(NotImplementedError, match=r"^train\.clip_opt\.tower_attention='wmma'"):
        train_config_from_opt(opt)


def test_the_metric_option_check_accepts_it(tmp_path):
    from satlas_super_resolution_amd import clipscore_metric as CM
    kw = dict(clip_model="clip-ViT-B/16", clip_weights=_clip_block(tmp_path)["clip_weights"])
    assert "tower_attention" in CM._OUR_KEYS
    absent = CM.check_clipscore_opt(**kw)
    assert CM.check_clipscore_opt(tower_attention="fma", **kw) == absent == CM.check_clipscore_opt(tower_attention="mfma", **kw)
    for bad in ("matrix", "Mfma", ""):
        with pytest.raises(NotImplementedError, match=f"calculate_clipscore.*tower_attention={bad!r}"):
            CM.check_clipscore_opt(tower_attention=bad, **kw)


@pytest.mark.parametrize("arith,attn", list(itertools.product((None, "exact", "split"), (None, "fma", "mfma"))))
def test_every_combination_with_tower_arithmetic_passes_the_checks(tmp_path, arith, attn):
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd import clipscore_metric as CM
    base = _clip_block(tmp_path)
    extra = {k: v for k, v in (("tower_arithmetic", arith), ("tower_attention", attn)) if v is not None}
    got = CL.check_clip_opt(dict(base, **extra))
    assert got.get("tower_arithmetic") == ("split" if arith == "split" else None)
    assert got.get("tower_attention") == ("mfma" if attn == "mfma" else None)
    CM.check_clipscore_opt(clip_model="siglip-ViT-SO400M-14", clip_weights=base["clip_weights"], **extra)


def test_the_source_the_header_and_hip_py_carry_the_entries():
    from satlas_super_resolution_amd import build, hip
    assert "mha_mfma.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "mha_mfma.hip"))
    header = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    for name, ret in zip(ENTRIES, ("int", "int64_t", "int")):
        assert re.search(rf"^{ret} {name}\(", header, re.M), name
        assert name in hip.ABI_SYMBOLS
    # the same argument lists as the entries beside which they stand
    args = lambda n: re.sub(r"\s+", " ", re.search(rf"^\w+ {n}\((.*?)\);", header, re.M | re.S).group(1))      # noqa: E731
    assert args("ssr_mha_mfma_fwd") == args("ssr_mha_fwd") and args("ssr_mha_mfma_bwd") == args("ssr_mha_bwd")
    assert args("ssr_mha_mfma_bwd_ws_floats") == args("ssr_mha_bwd_ws_floats")
    src = open(os.path.join(build.CSRC, "mha_mfma.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in src and all(f'extern "C" int{"64_t" if "ws" in n else ""} {n}(' in src for n in ENTRIES)
    misc = open(os.path.join(build.CSRC, "misc.hip")).read()
    assert re.search(r"ssr_abi_version\(void\)\s*{\s*return 3;", misc)                          # additive: the ABI version stays 3


def test_the_size_function_returns_int64_and_the_abi_version_is_3():
    from satlas_super_resolution_amd import hip
    import ctypes as C
    lib = hip.lib()
    assert lib.ssr_abi_version() == 3
    assert lib.ssr_mha_mfma_bwd_ws_floats.restype is C.c_int64
    assert lib.ssr_mha_mfma_bwd_ws_floats(2, 81, 3) == 3 * 2 * 81 * 3 and lib.ssr_mha_mfma_bwd_ws_floats(0, 81, 3) == -1
    assert lib.ssr_mha_mfma_bwd_ws_floats(65535, 1 << 20, 12) == 3 * 65535 * (1 << 20) * 12                    # past 2^31


def test_both_model_caches_distinguish_the_value():
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd import clipscore_metric as CM
    loss_keys = {CL._loss_model_key("/w.pth", "cuda:0", "tanh", arith, attn) for arith in ("exact", "split") for attn in ("fma", "mfma")}
    assert len(loss_keys) == 4
    metric_keys = {CM._model_key("siglip", "/w.pth", 0, "tanh", arith, attn) for arith in ("exact", "split") for attn in ("fma", "mfma")}
    assert len(metric_keys) == 4


def test_the_models_take_the_value_and_a_head_dim_outside_the_kernels_is_refused_by_name():
    import clipscore_fixture as FX
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd import clipscore_metric as CM
    from satlas_super_resolution_amd.linear_split import check_mfma_head_dim
    state = FX.tiny_state("clip")
    assert CM.CLIPVisualModel(state, "cpu").tower_attention == "fma"
    assert CM.CLIPVisualModel(state, "cpu", tower_attention="mfma").tower_attention == "mfma"
    with pytest.raises(NotImplementedError, match="calculate_clipscore.*tower_attention='x'"):
        CM.CLIPVisualModel(state, "cpu", tower_attention="x")
    import cliploss_fixture as LF
    assert CL.ClipLossModel(LF.tower_state("A"), "cpu").tower_attention == "fma"
    assert CL.ClipLossModel(LF.tower_state("A"), "cpu", tower_attention="mfma").tower_attention == "mfma"
    with pytest.raises(NotImplementedError, match=r"train\.clip_opt\.tower_attention='x'"):
        CL.ClipLossModel(LF.tower_state("A"), "cpu", tower_attention="x")
    check_mfma_head_dim(64, "here")
    check_mfma_head_dim(72, "here")
    for d in (8, 32, 80, 128):
        with pytest.raises(NotImplementedError, match=f"here: tower_attention 'mfma' takes head dims .*this tower has {d}"):
            check_mfma_head_dim(d, "here")
