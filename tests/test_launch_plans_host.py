"""CPU: the launch plans emit exactly what they emitted.

A plan (engine.GeneratorPlan / SplitGeneratorPlan / DiscriminatorPlan / ObjectBranchPlan, l2_archs.L2Plan) is data: lists of C-ABI calls
over descriptor records and tables.  tests/golden/launch_plans.json holds, per configuration x arithmetic mode x switch setting, the call
count and the sha256 of the canonical text tools/plan_transcript.py prints for it, recorded from the commit before the descriptor
builder, wgrad_plan.py and the weight-gradient schedule existed.  Every text is regenerated from the working tree (each switch setting
in a process of its own) and must be identical: there is no exception list.  The full text of one configuration is committed too, so
that a mismatch can be read as a diff."""
import ctypes as C
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
    with open(os.path.join(GOLDEN, "launch_plans.json")) as f:
        gold = json.load(f)
    return gold, pt.all_runs()


def test_every_plan_transcript_is_what_it_was(runs):
    gold, now = runs
    assert sorted(now) == sorted(gold["configs"])
    full = gold["full_text"][pt.FULL_TEXT]
    got = now[pt.FULL_TEXT][0].splitlines()
    assert got == full, "\n".join(list(difflib.unified_diff(full, got, "golden", "working tree", lineterm="", n=0))[:40])
    bad = [k for k, (text, calls) in now.items() if {"calls": calls, "sha256": pt.digest(text)} != gold["configs"][k]]
    assert not bad, "%d of %d transcripts differ from the golden file: %s" % (len(bad), len(now), bad[:12])


def test_the_sweep_is_not_hollow(runs):
    """every C entry point engine.py hands to a Launcher occurs in some transcript; paired and single items of both kinds, a non-empty
    reduce table, the split tables of the older fp32x3 form, forks, segments and every switch's own path occur"""
    _, now = runs
    src = open(os.path.join(ROOT, "satlas_super_resolution_amd", "engine.py")).read()
    named = set(re.findall(r"\.add\(\s*(?:hip\.lib\(\)|lib)\.(ssr_\w+)", src))
    assert len(named) >= 18, sorted(named)
    text = "\n".join(t for t, _ in now.values())
    called = set(re.findall(r"^\s*call (ssr_\w+) ", text, re.M))
    assert named <= called, sorted(named - called)
    items = re.findall(r"^  item \{.* atomic=(\d) nco=(\d) ", text, re.M)
    assert {("0", "1"), ("0", "2"), ("1", "1"), ("1", "2")} <= set(items), sorted(set(items))
    for needle in ("  reduce {", "  split pass 2 layer", "  split item {", " per-split ", "fork 'wgrad chunk' {", "fork 'another part of the batch' {",
                   "join", "bwd_segment 2 ", "call ssr_conv2d_chain ", "call ssr_conv2d_fixup ", "  gather seg {", "  sn bwd item {", "  pack bwd {"):
        assert needle in text, needle
    # a setting that changed nothing it was meant to change would be a hollow run: each differs from the unset run somewhere
    for setting in pt.RUNS[1:]:
        keys = [k for k in now if k.endswith("[%s]" % setting)]
        assert keys and any(now[k][0] != now[k.split(" [")[0]][0] for k in keys), setting
    assert len(now) == len(pt.RUNS[1:]) * sum(len(pt.CONFIGS[c][2]) for c in pt.SWITCHED) + sum(len(m) for _, _, m in pt.CONFIGS.values())


def _raw(records):
    return [bytes(memoryview(r).cast("B")) for r in records]


def _dense_blocks(hip, add, n_blocks, N, big=True):
    """the layers of tests/test_host_boundary.py's weight-gradient tests: dense blocks (conv1..conv5 read one 192-channel buffer) at
    32 x 32 and one 64 -> 64 layer at 128 x 128"""
    V, base = hip.View, 0x10000000
    for r in range(n_blocks):
        xb = base + r * 0x4000000
        for k in range(5):
            cin, cout = 64 + 32 * k, (64 if k == 4 else 32)
            dy = V(xb + 0x1000000, 192, 64 + 32 * k) if k < 4 else V(xb + 0x2000000, 192, 0)
            add(V(xb, 192, 0), dy, N, 32, 32, 1, cin, cout, 32, 32, 1.0, 0x5000 + 64 * (5 * r + k), cin, 0x6000)
    if big:
        add(V(base + 0x9000000, 64, 0), V(base + 0xa000000, 64, 0), N, 128, 128, 1, 64, 64, 128, 128, 1.0, 0x7000, 64, 0x8000)


@pytest.mark.parametrize("dtype,n_blocks,N", [("bf16", 2, 4), ("fp32x3", 1, 16), ("fp32x3", 24, 16)])
def test_planning_functions_on_plain_records_give_the_batch_its_items(dtype, n_blocks, N, monkeypatch):
    """wgrad_plan's functions need no WgradBatch, no torch and no device: from layer records and the kernels' tile counts they give,
    record for record, the items WgradBatch.add cuts and what its pairing, cost, makespan, balance and the three orders return - and
    those keep the properties tests/test_host_boundary.py asserts through a batch (nothing lost or doubled, pairs over one input
    patch, longest first, buffer groups on one XCD)."""
    from satlas_super_resolution_amd import engine, hip, wgrad_plan as wp
    for name in ("SSR_X3_WGRAD_FUSED", "SSR_WGRAD_ORDER"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(engine, "_device_cus", lambda: (256, 8))
    code, lib = hip.dtype_code(dtype), hip.lib()
    wb = engine.WgradBatch(code, 3, 1, device="cpu")
    _dense_blocks(hip, wb.add, n_blocks, N, big=n_blocks < 24)
    # the same layers as plain records, cut by the pure function
    layers, items = [], []

    def add(x, dy, N, hi, wi, up, cin, cout, gh, gw, alpha, dw, cin_w, db):
        tiles = lib.ssr_wgrad_tiles(N, gh, gw, wb.kdt, 3)
        splits = max(1, -(-tiles // (128 * (2 if wb.kdt == hip.F32X3 else 1))))
        layers.append(hip.WgradLayer(x, dy, N, hi, wi, up, cin, cout, 1, 1, gh, gw, alpha, dw, cin_w, db))
        items.extend(wp.cut([len(layers) - 1] * splits, cout, cin_w, lib.ssr_wgrad_ci_tile(wb.kdt, 3), tiles, 1 if splits > 1 else 0))
    _dense_blocks(hip, add, n_blocks, N, big=n_blocks < 24)
    assert _raw(layers) == _raw(wb.layers) and _raw(items) == _raw(wb.items) and len(items) > 0
    paired = wp.pair(layers, items)
    assert _raw(paired) == _raw(wb._pair(wb.items))
    assert [wp.cost(it) for it in paired] == [wb._cost(it) for it in paired]
    assert wp.makespan(paired, 256) == wb._makespan(paired)
    balanced, choice = wp.balance(paired, 256)
    assert _raw(balanced) == _raw(wb._balance(paired)) and choice == wb.balance_choice
    assert wp.makespan(balanced, 256) <= wp.makespan(paired, 256) == choice[3]
    assert _raw(wp.ORDERS["hybrid"](layers, paired, 8)) == _raw(wb._cost_xcd_order(paired))
    assert sorted(wp.ORDERS) == ["heavy", "hybrid", "xcd"]
    # pairing: every (layer, co block, ci chunk, pixel range) exactly once, pairs share the input patch
    key = lambda it: (it.layer, it.co0, it.ci0, it.tile_begin, it.tile_end)      # noqa: E731
    seen = [key(it) for it in paired] + [(it.layer_b, it.co0_b, it.ci0, it.tile_begin, it.tile_end) for it in paired if it.nco == 2]
    assert sorted(seen) == sorted(map(key, items)) and len(set(seen)) == len(seen)
    for it in paired:
        if it.nco == 2:
            A, B = layers[it.layer], layers[it.layer_b]
            assert (A.x.p, A.x.cs, A.x.coff, A.N, A.Hi, A.Wi, A.Gh, A.Gw) == (B.x.p, B.x.cs, B.x.coff, B.N, B.Hi, B.Wi, B.Gh, B.Gw)
            assert (min(64, A.Cin_w - it.ci0) > 32) == (min(64, B.Cin_w - it.ci0) > 32) and (it.layer, it.co0) != (it.layer_b, it.co0_b)
    assert sum(it.nco == 2 for it in paired if it.layer < 5) == 6 and sum(it.nco != 2 for it in paired if it.layer < 5) == 2
    # every order is a permutation; heavy and hybrid are sorted by cost; hybrid keeps a buffer group of one cost on one XCD (block % 8)
    full = lambda it: key(it) + (it.nco, it.layer_b, it.co0_b)      # noqa: E731
    for name, fn in wp.ORDERS.items():
        got = fn(layers, paired, 8)
        assert sorted(map(full, got)) == sorted(map(full, paired)), name
        costs = [wp.cost(it) for it in got]
        if name != "xcd":
            assert costs == sorted(costs, reverse=True) and got[0].nco == 2, name
        if name == "hybrid" and n_blocks == 24:
            groups = {}
            for pos, it in enumerate(got):
                groups.setdefault((wp.cost(it), layers[it.layer].x.p), []).append(pos % 8)
            same = sum(len(set(xs)) == 1 for xs in groups.values())
            assert same >= 0.9 * len(groups), (name, same, len(groups))
    assert C.sizeof(hip.WgradItem) == 36 and all(wp.weight(layers, it) > 0 for it in paired)


def test_switches_are_read_through_one_helper_and_descriptors_built_in_one_place():
    """the structure the refactor left: os.environ only behind hip.env_*, ConvDesc constructed in conv_desc() and in the array copy,
    WgradLayer in WgradBatch.add and the twin-plane copy, no nonlocal, and l2_archs assigns no field of a layer record"""
    pkg = os.path.join(ROOT, "satlas_super_resolution_amd")
    src = {n: open(os.path.join(pkg, n)).read() for n in ("engine.py", "wgrad_plan.py", os.path.join("archs", "l2_archs.py"), "hip.py")}
    for n in ("engine.py", "wgrad_plan.py"):
        assert "os.environ" not in src[n] and "nonlocal" not in src[n], n
    both = src["engine.py"] + src[os.path.join("archs", "l2_archs.py")]
    assert len(re.findall(r"\bConvDesc\(\)", both)) == 1 and len(re.findall(r"\(ConvDesc \* ", both)) == 1
    assert len(re.findall(r"\bWgradLayer\(", src["engine.py"])) == 2 and "WgradLayer" not in src[os.path.join("archs", "l2_archs.py")]
    assert not re.search(r"\.pad_[yx]\s*=", src[os.path.join("archs", "l2_archs.py")])
    assert len(re.findall(r"os\.environ", src["hip.py"])) == 4
