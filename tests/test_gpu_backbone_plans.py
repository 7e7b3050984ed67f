"""GPU: the backbone plans built on the device, with the real ParamStore.pack(), are the ones tests/golden/backbone_plans.json records
from the CPU (tests/test_backbone_plans_host.py compares every configuration there).  Nothing is launched but ssr_pack_weights."""
import difflib
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_transcript as pt  # noqa: E402


def tensors_of(plan):
    out = [plan.store.data, plan.xn]
    for v in vars(plan).values():
        out += [v] if isinstance(v, torch.Tensor) else [t for t in v.values() if isinstance(t, torch.Tensor)] if isinstance(v, dict) else []
    return out


@pytest.mark.parametrize("name", pt.BACKBONE_FULL_TEXT)
def test_backbone_plans_built_on_the_device_match_the_golden_transcripts(name):
    assert name.split("/")[0] in ("lpips", "perceptual")
    with open(os.path.join(GOLDEN, "backbone_plans.json")) as f:
        gold = json.load(f)
    plan, launchers, weights, extra = pt.backbone_objects(name, "cuda")
    assert all(t.is_cuda for t in tensors_of(plan)) and all(t.is_cuda for _, t in weights) and len(tensors_of(plan)) > 12
    text, calls = pt.backbone_transcript(plan, launchers, weights, extra)
    full, got = gold["full_text"][name], text.splitlines()
    assert got == full, "\n".join(list(difflib.unified_diff(full, got, "golden", "device", lineterm="", n=0))[:40])
    assert {"calls": calls, "sha256": pt.digest(text)} == gold["configs"][name]
