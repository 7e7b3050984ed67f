"""CPU: which kernel family ssr_conv2d picks for a descriptor, and under which symbol it reports the launch, is what it was.

tests/golden/conv_dispatch_table.json holds what ssr_conv2d_variant / ssr_conv2d_symbol answered for 20 160 descriptors before the
dispatch became one table (csrc/conv_dispatch.h, select() in csrc/conv.hip) - once with no switch set and once per off switch, each in
a process of its own (tools/make_conv_dispatch_golden.py; nothing is launched).  The table is regenerated from the built library and
every row must be identical, except where the old reports did not say what ssr_conv2d launched: REWRITES, one rule per drift."""
import json
import os
import re
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_conv_dispatch_golden as sweep  # noqa: E402

F32, BF16, F32X3, F32H3 = 0, 1, 2, 3
TABLE = os.path.join(GOLDEN, "conv_dispatch_table.json")


@pytest.fixture(scope="module")
def runs():
    import __graft_entry__ as ge
    ge.build()
    with open(TABLE) as f:
        gold = sweep.decode(json.load(f))
    return gold, sweep.all_runs()


def _split_pipelined_tile(setting, what, gold):
    # the split-mode pipelined launch overrides the half-height tile with SSR_X3_SMALL (default 0: never): MW = 4 runs, W2 was reported
    dtype, K = what[0], what[1]
    if dtype in (F32X3, F32H3) and K != 4 and re.search(r"conv_[xh]3_kernel<.*,W2>$", gold):
        v, sym = gold.split("|")
        return "%d|%s" % (int(v) + 2, sym.replace(",W2>", ",W4>"))
    return gold


def _split_stride2_runs_exact_fp32(setting, what, gold):
    # split-mode 4x4 stride-2 layers without s2d are retargeted to the exact fp32 kernel: conv_kernel<fp32,...> runs, conv_x3 / conv_h3 was reported
    dtype, K, extra = what[0], what[1], what[7]
    if dtype in (F32X3, F32H3) and K == 4 and "s2d" not in extra:
        return re.sub(r"conv_[xh]3_kernel<fp32(x3|h),", "conv_kernel<fp32,", gold)
    return gold


def _deep_pipeline_opt_in(setting, what, gold):
    # SSR_X3_PIPE=1 sends the 32-channel-tile fp32x3 layers whose stages come from one view to conv_x3p_kernel: no report knew that family
    dtype, Cin, extra = what[0], what[2], what[7]
    if setting == "SSR_X3_PIPE=1" and dtype == F32X3 and ",NT1,W4>" in gold and not ("x2" in extra and Cin % 32):
        return gold.replace("conv_x3_kernel<", "conv_x3p_kernel<")
    return gold


def _s2d_input_beyond_32_bit_offsets(setting, what, gold):
    # a space-to-depth layer whose input the split big-tile kernel cannot address (> 2^31 - 256 bytes): ssr_conv2d returns SSR_EUNSUP
    # without a launch, and now both queries return it too; digit 9 / conv_big?3_kernel4<2> was reported
    dtype, Cin, grid, N, extra = what[0], what[2], what[4], what[5], what[7]
    if dtype in (F32X3, F32H3) and "s2d" in extra and (N * (2 * grid) ** 2 + 2 * grid + 1) * Cin * 4 > 0x7fffff00:
        return "-2|rc=-2"
    return gold


REWRITES = [_split_pipelined_tile, _split_stride2_runs_exact_fp32, _deep_pipeline_opt_in, _s2d_input_beyond_32_bit_offsets]


def test_golden_table_is_small_and_complete():
    assert os.path.getsize(TABLE) <= 256 * 1024
    with open(TABLE) as f:
        doc = json.load(f)
    assert sorted(doc["runs"]) == sorted(sweep.RUNS) and doc["rows"] >= 20000


def test_every_row_is_the_parents_except_the_listed_drifts(runs):
    gold, new = runs
    rewritten = {r.__name__: 0 for r in REWRITES}
    bad = []
    for setting in sweep.RUNS:
        rows, what = new[setting]["rows"], new[setting]["what"]
        assert len(rows) == len(gold[setting])
        for i, (g, got) in enumerate(zip(gold[setting], rows)):
            want = g
            for rule in REWRITES:
                nxt = rule(setting, what[i], want)
                rewritten[rule.__name__] += nxt != want
                want = nxt
            if got != want:
                bad.append((setting, what[i], g, want, got))
    assert not bad, (len(bad), bad[:10])
    assert all(rewritten.values()), rewritten              # every rule is exercised: a rule nothing needs is a rule to delete


def test_sweep_reaches_every_family(runs):
    """every last digit of the variant code occurs: 1 resident, 2 / 4 pipelined, 5 register-tiled, 6 ring (only with SSR_X3_REGTILE=0),
    7 thin-output, 8 weight-stationary, 9 big tile"""
    gold, new = runs
    for table in (gold, {k: r["rows"] for k, r in new.items()}):
        digits = {int(row.split("|")[0]) % 10 for rows in table.values() for row in rows}
        assert digits >= {1, 2, 4, 5, 6, 7, 8, 9}, digits
    assert {int(r.split("|")[0]) % 10 for r in new["SSR_X3_REGTILE=0"]["rows"]} >= {6}
    assert 6 not in {int(r.split("|")[0]) % 10 for r in new[""]["rows"]}


def test_weight_stationary_report_follows_the_launch():
    """A drift the sweep's rotation of epilogues does not reach: the weight-stationary launch declines 64-channel layers with a residual /
    mask epilogue and a 32-channel padded width (they would spill), ssr_conv2d goes on down the list - and digit 8 was reported.  The
    decline is part of the family's `qualifies` now: the report names the pipelined kernel that runs."""
    import ctypes as C
    from satlas_super_resolution_amd import hip
    for extra, digit in (("", 8), ("r1", 4), ("m", 4)):
        d = sweep.make_desc(hip, BF16, 3, 1, 64, 32, 128, 32, hip.ACT_NONE, extra)
        assert hip.lib().ssr_conv2d_variant(C.byref(d)) == 3110 + digit, extra
