"""CPU: the LPIPS metric plans (VGG16, AlexNet) and the perceptual loss plan (VGG19) emit exactly what they emitted.

tests/golden/backbone_plans.json holds, per configuration of tools/plan_transcript.py's BACKBONE_CONFIGS, the call count and the sha256
of the canonical text - every launcher call by call, the plan's ParamStore (and a sha256 over its fp32 arena), every other device
weight (key, shape, dtype, one sha256 over the bytes), the element count of every buffer the plan owns - and the sha256 of three random
states, recorded from the commit before cnn_backbone.py existed, when perceptual.py and lpips_metric.py wrote the backbone out three
times.  Every text is regenerated from the working tree and must be identical: there is no exception list.  The full text of one
AlexNet and one perceptual configuration is committed too, so that a mismatch can be read as a diff.

No image size makes ssr_conv2d refuse one of AlexNet's 3 x 3 layers (the pipelined family takes every grid of a 3 x 3 stride-1 layer in
exact fp32), so the plan's fallback to ssr_conv_direct is recorded by lpips/alex/31x31/refused, in which the tool answers
ssr_conv2d_variant with SSR_EUNSUP itself."""
import difflib
import json
import os
import re
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_transcript as pt  # noqa: E402

FILES = ("cnn_backbone.py", "lpips_metric.py", "perceptual.py")


@pytest.fixture(scope="module")
def runs():
    import __graft_entry__ as ge
    ge.build()
    with open(os.path.join(GOLDEN, "backbone_plans.json")) as f:
        gold = json.load(f)
    return gold, pt.backbone_sweep()


def calls_of(text, launcher=None):
    """the C entry points of a text in order, of every launcher or of one"""
    if launcher is not None:
        text = text.split("launcher %s\n" % launcher)[1].split("\nlauncher ")[0].split("\nstore ")[0]
    return re.findall(r"^\s*call (ssr_\w+) ", text, re.M)


def test_every_backbone_transcript_is_what_it_was(runs):
    gold, now = runs
    assert sorted(now) == sorted(gold["configs"]) and sorted(gold["full_text"]) == sorted(pt.BACKBONE_FULL_TEXT)
    for name in pt.BACKBONE_FULL_TEXT:
        full, got = gold["full_text"][name], now[name][0].splitlines()
        assert got == full, "\n".join(list(difflib.unified_diff(full, got, "golden", "working tree", lineterm="", n=0))[:40])
    bad = [k for k, (text, calls) in now.items() if {"calls": calls, "sha256": pt.digest(text)} != gold["configs"][k]]
    assert not bad, "%d of %d transcripts differ from the golden file: %s" % (len(bad), len(now), bad[:12])


def test_the_random_states_draw_in_the_recorded_order(runs):
    gold, _ = runs
    assert len(gold["random_states"]) == 3 and pt.random_state_hashes() == gold["random_states"]


def test_the_backbone_sweep_is_not_hollow(runs):
    """every C entry point the three files hand to a Launcher (named through `lib.` and not called on the spot) occurs in some
    transcript, the call counts are the expected constants, and each option's text differs from its base in the way the option is meant
    to change it"""
    _, now = runs
    pkg = os.path.join(ROOT, "satlas_super_resolution_amd")
    src = "".join(open(os.path.join(pkg, n)).read() for n in FILES)
    named = set(re.findall(r"\blib\.(ssr_\w+)\b(?!\()", src))
    assert len(named) == 11, sorted(named)
    text = lambda name: now[name][0]                                        # noqa: E731
    called = set(calls_of("\n".join(t for t, _ in now.values())))
    assert named <= called and "ssr_conv2d" in called, sorted(named - called)
    assert len(now) == 2 + 5 + 5 + 6
    # VGG16: 2 inputs, 13 convolutions, 4 relu+pool, 5 taps; AlexNet: 2 inputs, 5 convolutions, 2 poolings, 5 taps
    # VGG19 up to conv5_4: per forward 1 normalise + 16 convolutions + 4 relu+pool = 21; bwd 5 L1 + 16 dgrads + 4 relu+pool + 1 normalise = 26
    # up to conv3_4: 2 x (1 + 8 + 2) + (3 + 8 + 2 + 1);  style: + 5 gram in fwd_target, + 10 in fwd, + 5 in bwd;  style only: - 5 L1
    want = {"lpips/vgg": 24, "lpips/alex": 14, "perceptual": 68, "perceptual/fp32/conv3_4": 36, "perceptual/fp32/style": 88, "perceptual/fp32/style_only": 83}
    for name, (_, calls) in now.items():
        key = name if name in want else "/".join(name.split("/")[:2]) if name.startswith("lpips") else "perceptual"
        assert calls == want[key], (name, calls)
    base = text("perceptual/fp32")
    for name in now:
        if name.startswith("perceptual/") and name != "perceptual/fp32":
            assert text(name) != base, name
        if name.startswith("perceptual/"):
            assert calls_of(text(name), "fwd_target")[:2] == ["ssr_channel_affine", "ssr_conv2d"] and calls_of(text(name), "bwd")[-1] == "ssr_channel_affine"
    # style adds the Gram launches; perceptual_weight 0 with style removes the feature L1 and makes the Gram backward overwrite
    assert not [c for c in calls_of(base) if c.startswith("ssr_gram_")]
    style, only = text("perceptual/fp32/style"), text("perceptual/fp32/style_only")
    assert calls_of(style, "fwd_target")[-5:] == ["ssr_gram_fwd"] * 5 and calls_of(style, "fwd")[-10:] == ["ssr_gram_fwd", "ssr_gram_l1"] * 5
    assert calls_of(style, "bwd")[:10] == ["ssr_l1_loss", "ssr_gram_bwd"] * 5 and calls_of(only, "bwd")[:5] == ["ssr_gram_bwd"] * 5
    assert "ssr_l1_loss" not in calls_of(only) and calls_of(only, "fwd") == calls_of(style, "fwd")
    assert len(re.findall(r"call ssr_gram_bwd .* 1$", style, re.M)) == 5 and len(re.findall(r"call ssr_gram_bwd .* 0$", only, re.M)) == 5
    # the truncated tap set: 8 convolutions per forward, 8 dgrads, a store of 8 layers
    short = text("perceptual/fp32/conv3_4")
    assert calls_of(short).count("ssr_conv2d") == 3 * 8 and calls_of(base).count("ssr_conv2d") == 3 * 16
    assert short.count("\n  pack {") == 8 and base.count("\n  pack {") == 16 and "features.16" in short and "features.19" not in short
    # the normalisation affine: mean / std, none, range_norm; the deterministic flag in the dtype of ssr_l1_loss only
    affine = lambda t: re.findall(r"call ssr_channel_affine 'vgg normalise' .* (\[\S+\] \[\S+\]) 0$", t, re.M)        # noqa: E731
    one, zero, half = pt._fbits(1.0), pt._fbits(0.0), pt._fbits(0.5)
    assert affine(text("perceptual/fp32/no_input_norm")) == ["[%s] [%s]" % (",".join([one] * 3 + [zero] * 5), ",".join([zero] * 8))] * 2
    assert len({affine(text("perceptual/fp32" + n))[0] for n in ("", "/no_input_norm", "/range_norm")}) == 3
    assert half not in affine(base)[0] and zero in affine(base)[0]
    det = text("perceptual/fp32/deterministic")
    from satlas_super_resolution_amd import hip
    assert len(re.findall(r"call ssr_l1_loss '[^']*' \S+ \S+ \S+ %d " % hip.DETERMINISTIC, det)) == 5
    assert re.sub(r"(call ssr_l1_loss '[^']*' \S+ \S+ \S+) %d " % hip.DETERMINISTIC, r"\1 0 ", det) == base
    # the arithmetic modes: the dtype codes of the store, five different texts
    assert len({text("perceptual/" + m) for m in pt.MODES}) == 5
    for m in pt.MODES:
        code = hip.dtype_code(m)
        assert ("store ParamStore dtype=%d fwd_dtype=%d " % (hip.storage_code(code), hip.forward_code(code))) in text("perceptual/" + m), m
    # LPIPS feeds: the permutation array and the flag of ssr_lpips_input, nothing else
    for bgr, rgb in (("lpips/vgg/bgr", "lpips/vgg/rgb+normalize"), ("lpips/alex/64x64", "lpips/alex/64x64/rgb+normalize")):
        assert text(bgr).count(" [2,1,0] 0\n") == 2 and text(rgb).count(" [0,1,2] 1\n") == 2
        assert text(bgr).replace(" [2,1,0] 0\n", " [0,1,2] 1\n") == text(rgb)
    # AlexNet: taps of 7, 3, 1, 1, 1 at the smallest side; a 3 x 3 layer in both forms
    assert re.findall(r"call ssr_lpips_layer '[^']*' \S+ \S+ \S+ 0 2 (\d+) ", text("lpips/alex/31x31")) == ["49", "9", "1", "1", "1"]
    assert len({text("lpips/alex/%s" % s) for s in ("31x31", "35x47", "64x64")}) == 3
    for name in ("31x31", "35x47", "64x64"):
        assert calls_of(text("lpips/alex/" + name)).count("ssr_conv2d") == 3 and calls_of(text("lpips/alex/" + name)).count("ssr_conv_direct") == 2
    refused = text("lpips/alex/31x31/refused")
    assert calls_of(refused).count("ssr_conv_direct") == 5 and "ssr_conv2d" not in calls_of(refused)
    assert "call ssr_conv_direct 'conv direct conv3' " in refused and "call ssr_conv2d 'conv fwd features.6' " in text("lpips/alex/31x31")
    assert [c for c in calls_of(refused) if "conv" not in c] == [c for c in calls_of(text("lpips/alex/31x31")) if "conv" not in c]


def test_the_backbone_is_written_once():
    """the structure the refactor left: the fused ReLU + pooling pass, the 3 x 3 pooling, the direct convolution and the question that
    decides on the direct fallback are each named in one file of the package"""
    pkg = os.path.join(ROOT, "satlas_super_resolution_amd")
    src = {n: open(os.path.join(pkg, n)).read() for n in sorted(os.listdir(pkg)) if n.endswith(".py")}
    for pattern in (r"lib\.ssr_relu_maxpool2_fwd\b", r"lib\.ssr_maxpool3s2_fwd\b", r"lib\.ssr_conv_direct\b", r"lib\.ssr_conv2d_variant\b"):
        assert [n for n, text in src.items() if re.search(pattern, text)] == ["cnn_backbone.py"], pattern
