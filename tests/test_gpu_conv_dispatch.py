"""GPU: what ssr_conv2d_variant reports is what ssr_conv2d launches.

For every kernel family and every dtype it serves, the smallest N = 1 layer that the library sends to the family by itself (found with
the CPU query, tools/conv_dispatch_ab.py find_case) runs through ssr_conv2d and through ssr_conv2d_impl with the family forced: the
bytes must be equal.  The same layer on the next family down the list that can run it is another kernel: it must agree within the
tolerance the parity tests hold that pair to, and is not required to be byte-equal.  No profiler and no golden bytes."""
import os
import sys

import pytest
import torch

from conftest import ROOT, rel_err

sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_dispatch_ab as ab  # noqa: E402

pytestmark = pytest.mark.gpu

# Two kernels are each held to TOL of max|ref| against the float64 contract reference (tests/test_gpu_conv_x3.py: fp32x3 1e-4; exact fp32
# and the fp16 split 2e-6), so they are within 2 TOL of each other; bf16 pairs are compared directly at 1e-2 (tests/test_gpu_parity.py
# test_stride2_dgrad_big_tile_parity_classes).
PAIR_TOL = {"fp32x3": 2 * 1e-4, "fp32": 2 * 2e-6, "fp32h": 2 * 2e-6, "bf16": 1e-2}


def _impl(family):
    """the ssr_conv2d_impl code that reaches a family: its own, or 2 (every family that cannot be forced: the resident kernel)"""
    code = ab.FAMILY[family][1]
    return 2 if code is None else code


def _cases():
    import __graft_entry__ as ge
    ge.build()                                                 # (collection asks the library which layer goes where)
    from satlas_super_resolution_amd import hip
    return [pytest.param(mode, family, c, id=f"{mode}-{family}") for mode, family, c in ab.cases(hip)]


@pytest.mark.parametrize("mode,family,case", _cases())
def test_report_is_the_launch(mode, family, case):
    layer = ab.Layer(mode, *case)
    auto, forced = layer.run(0), layer.run(_impl(family))
    assert forced is not None, "the family the query names refuses the layer"
    assert float(auto.float().abs().max()) > 0
    assert torch.equal(auto.view(torch.uint8), forced.view(torch.uint8)), (mode, family, case)
    order = ab.ORDER[mode]
    for below in order[order.index(family) + 1:]:
        other = layer.run(_impl(below))
        if other is None:                                      # SSR_EUNSUP: that family cannot run this layer at all, the next one down
            continue
        e = rel_err(other, auto)
        print(f"{mode} {family} vs {below} forced: {e:.3g} (bound {PAIR_TOL[mode]:g})")
        assert e <= PAIR_TOL[mode], (mode, family, below, e)
        break


def test_every_family_row_has_a_case():
    """the ring kernel is the one row the library never picks by itself (the register-tiled kernel takes every layer it could run): it is
    covered as the family below x3r in fp32x3"""
    from satlas_super_resolution_amd import hip
    have = {(mode, family) for mode, family, _ in ab.cases(hip)}
    want = {(mode, family) for mode, order in ab.ORDER.items() for family in order}
    assert want - have == {("fp32x3", "x3q")}
