"""GPU: the tower plans built on the device, with the real weight packing, are the ones tests/golden/tower_plans.json records from the
CPU (tests/test_tower_plans_host.py compares every configuration there).  Nothing is launched but ssr_linear_split_pack at model
construction."""
import difflib
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_transcript as pt  # noqa: E402


@pytest.mark.parametrize("name", pt.TOWER_FULL_TEXT)
def test_tower_plans_built_on_the_device_match_the_golden_transcripts(name):
    assert name.split("/")[0] in ("metric", "loss") and "/split/mfma/" in name
    with open(os.path.join(GOLDEN, "tower_plans.json")) as f:
        gold = json.load(f)
    fn, kw = pt.TOWER_CONFIGS[name]
    model, plan, launchers, extra = fn("cuda", **kw)
    assert all(t.is_cuda for t in model.w.values()) and all(t.is_cuda for t in plan.bufs.values()) and any(k.endswith(".pk") for k in model.w)
    text, calls = pt.tower_transcript(model, plan, launchers, extra)
    full, got = gold["full_text"][name], text.splitlines()
    assert got == full, "\n".join(list(difflib.unified_diff(full, got, "golden", "device", lineterm="", n=0))[:40])
    assert {"calls": calls, "sha256": pt.digest(text)} == gold["configs"][name]
