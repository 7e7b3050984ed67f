"""GPU: the launch plans built on the device are the ones tests/golden/launch_plans.json records (tests/test_launch_plans_host.py
compares every configuration on the CPU), and every descriptor table on the device holds the host records it was made from.
Nothing is launched."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_transcript as pt  # noqa: E402


@pytest.mark.parametrize("name,mode", [("gen_train", "fp32x3"), ("gen_det", "fp32x3"), ("disc128_in3_skip", "fp32x3")])
def test_plans_built_on_the_device_match_the_golden_transcripts(name, mode, monkeypatch):
    from satlas_super_resolution_amd import engine
    for k in [k for k in os.environ if k.startswith("SSR_")]:
        monkeypatch.delenv(k)
    monkeypatch.setattr(engine, "_device_cus", engine._device_cus)        # objects() pins it to (256, 8): put back afterwards
    assert not engine.X3_FIXUP[0] and not engine.deterministic()          # (read at import)
    with open(os.path.join(GOLDEN, "launch_plans.json")) as f:
        gold = json.load(f)["configs"]["%s/%s" % (name, mode)]
    plans, stores, extra = pt.objects(name, mode, "cuda")
    assert all(st.data.is_cuda for st in stores)
    text, calls = pt.transcript(plans, stores, extra)
    assert {"calls": calls, "sha256": pt.digest(text)} == gold
    tables = pt.tables_of(plans, stores)
    assert len(tables) >= 3
    if name == "gen_det":
        assert any(what.endswith("reduce") for what, _, _ in tables)
    for what, tab, records in tables:
        assert tab.is_cuda and len(records) > 0, what
        assert tab.cpu().numpy().tobytes() == b"".join(bytes(memoryview(r).cast("B")) for r in records), what
