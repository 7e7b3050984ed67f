"""CPU: the CLIPScore metric plan and the CLIP loss plan emit exactly what they emitted.

tests/golden/tower_plans.json holds, per configuration of tools/plan_transcript.py's TOWER_CONFIGS, the call count and the sha256 of
the canonical text - every launcher call by call, the model's weight list (with a sha256 over the bytes under exact arithmetic), the
plan's buffer elements and the loss plan's saved_bytes - recorded from the commit before vit_tower.py existed, when each of the two
plans wrote the tower out on its own.  Every text is regenerated from the working tree and must be identical: there is no exception
list.  The full text of one metric and one loss configuration is committed too, so that a mismatch can be read as a diff."""
import difflib
import json
import os
import re
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_transcript as pt  # noqa: E402


@pytest.fixture(scope="module")
def runs():
    import __graft_entry__ as ge
    ge.build()
    with open(os.path.join(GOLDEN, "tower_plans.json")) as f:
        gold = json.load(f)
    return gold, pt.tower_sweep()


def test_every_tower_transcript_is_what_it_was(runs):
    gold, now = runs
    assert sorted(now) == sorted(gold["configs"]) and sorted(gold["full_text"]) == sorted(pt.TOWER_FULL_TEXT)
    for name in pt.TOWER_FULL_TEXT:
        full, got = gold["full_text"][name], now[name][0].splitlines()
        assert got == full, "\n".join(list(difflib.unified_diff(full, got, "golden", "working tree", lineterm="", n=0))[:40])
    bad = [k for k, (text, calls) in now.items() if {"calls": calls, "sha256": pt.digest(text)} != gold["configs"][k]]
    assert not bad, "%d of %d transcripts differ from the golden file: %s" % (len(bad), len(now), bad[:12])


def test_the_tower_sweep_is_not_hollow(runs):
    """every C entry point clip_loss.py, clipscore_metric.py and vit_tower.py hand to a Launcher (named through `lib.` and not called
    on the spot) occurs in some transcript, the sweep is the table it was set to be, and each option setting's text differs from the
    default's"""
    _, now = runs
    pkg = os.path.join(ROOT, "satlas_super_resolution_amd")
    src = "".join(open(os.path.join(pkg, n)).read() for n in ("clip_loss.py", "clipscore_metric.py", "vit_tower.py"))
    named = set(re.findall(r"\blib\.(ssr_\w+)\b(?!\()", src)) - {"ssr_mha_bwd_ws_floats", "ssr_mha_mfma_bwd_ws_floats"}   # sizes, chosen by name
    assert len(named) == 15, sorted(named)
    text = "\n".join(t for t, _ in now.values())
    called = set(re.findall(r"^\s*call (ssr_\w+) ", text, re.M))
    assert named <= called, sorted(named - called)
    assert len(now) == 2 * 2 * 2 * (2 + 1) + 1                      # towers x arithmetics x attentions x (two metric families + the loss) + raw feed
    for kind, calls in (("metric/siglip", 25), ("metric/clip", 20), ("loss", 2 * 83)):       # the loss: three lists and their concatenation
        got = {c for k, (_, c) in now.items() if k.startswith(kind + "/")}
        assert got == {calls}, (kind, got)
    base = "metric/siglip/exact/fma/d64"
    for other in ("metric/siglip/split/fma/d64", "metric/siglip/exact/mfma/d64", "metric/clip/exact/fma/d64", "metric/siglip/exact/fma/d64/raw",
                  "metric/siglip/exact/fma/d72"):
        assert now[other][0] != now[base][0], other
    for other in ("loss/split/fma/d64", "loss/exact/mfma/d64", "loss/exact/fma/d72"):
        assert now[other][0] != now["loss/exact/fma/d64"][0], other
    raw, fed = now[base + "/raw"][0], now[base][0]
    assert " [0,1,2] null null\n" in raw and " [2,1,0] [f:" in fed and "null null\n" not in fed
    for name, (t, _) in now.items():                               # what each setting is meant to change is what changes
        parts = name.split("/")
        assert ("call ssr_linear_split " in t) == ("split" in parts) and ("call ssr_linear " in t) == ("exact" in parts), name
        assert ("call ssr_mha_mfma_fwd " in t) == ("mfma" in parts) and ("weights sha256 " in t) == ("exact" in parts), name
        assert ("call ssr_mha_mfma_bwd " in t) == ("mfma" in parts and parts[0] == "loss") and ("saved_bytes " in t) == (parts[0] == "loss"), name
        tokens = 10 if "clip" in parts else 9                      # the blocks' attention: B, T, T, heads, head dim
        assert (" 2 %d %d 2 %d f:" % (tokens, tokens, 72 if "d72" in parts else 64)) in t, name


def test_the_new_argument_kinds_print_by_value():
    """a null pointer argument, a ctypes array of scalars and a double, as fmt_launcher prints them"""
    import ctypes as C
    from satlas_super_resolution_amd import engine, hip
    lib = hip.lib()
    v, L = hip.View(None, 0, 0), engine.Launcher()
    L.add(lib.ssr_vit_patch_input, None, 1, 2, 3, None, None, 4, 5, v, hip.F32, (C.c_int32 * 3)(2, 1, 0), (C.c_float * 3)(0.5, 1.0, 2.0), None, what="a")
    L.add(lib.ssr_layernorm_fwd, v, None, None, v, hip.F32, 6, 7, 1e-6, what="b")
    out = []
    assert pt.fmt_launcher(pt.Canon([]), L, out) == 2
    assert out == ["call ssr_vit_patch_input 'a' null 1 2 3 null null 4 5 (null,0,0) 0 [2,1,0] [f:3f000000,f:3f800000,f:40000000] null",
                   "call ssr_layernorm_fwd 'b' (null,0,0) null null (null,0,0) 0 6 7 d:3eb0c6f7a0b5ed8d"]


def test_the_tower_is_written_once():
    """the structure the refactor left: the exact | split product, the blocks' mfma forward and the weight packing are each named in
    one file of the package"""
    pkg = os.path.join(ROOT, "satlas_super_resolution_amd")
    src = {n: open(os.path.join(pkg, n)).read() for n in sorted(os.listdir(pkg)) if n.endswith(".py")}
    for pattern in (r"lib\.ssr_linear_split\b", r"lib\.ssr_mha_mfma_fwd\b", r"(?<!def )\bpack_tower\("):
        assert [n for n, text in src.items() if re.search(pattern, text)] == ["vit_tower.py"], pattern
