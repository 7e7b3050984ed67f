"""GPU: every convolution family of the dispatch table - thin, ws, big, bigx3 / bigh3, x3r, x3q, res, pipelined - in every
mode it serves, forward and data gradient, held to EXACT sums.  The operands lie on the dyadic lattices of tests/conv_lattice.py, for
which every product and every partial sum of every summation order is an fp32 number: the MFMA accumulation, the chunk and ring order,
the K-quarter sum and the persistent image stream must all give the bits of the float64 contract reference, lo pieces included.

Every case asserts (1) torch.equal against the float64 value on y, y0 and y1 - or membership in the candidate set where two or three
terms follow a rounded LeakyReLU value (conv_lattice.finish); (2) every sentinel around the output views bit-unchanged (other channels
of the buffer, a pixel row above and below) and x, x2, r1, r2, m bit-unchanged; (3) the symbol of the forced launch
(ssr_conv2d_symbol_impl) names the family, so that a case cannot silently run on another kernel (single launches; the parity classes go
through ssr_conv2d_batch, which has no such report: see test_stride2_dgrad_parity_classes).  Input channels that no view covers
and the pixel rows around the input are NaN: an over-read that reaches an accumulator poisons the result.  The exactness condition of
every case is asserted by conv_lattice.expected (and for the whole list, on the CPU, by tests/test_conv_lattice_host.py).

Per family and mode: a grid below one tile, exactly one tile, one tile plus one pixel in both directions, a chunk tail (Cin % 16 == 8, or
% 32 for the bf16 kernels), Cin_w < Cin, Cout that is no multiple of 32, every epilogue variant on one mid shape, sliced outputs.  Named
exceptions: ws and thin take at most 64 input channels, thin at most 8 output channels (K = 1728 is no layer of theirs); big needs 32
input channels and up; res holds at most six chunks and cannot be forced (its list is what fits: conv_lattice.res_fits); the big-tile
families need CoutPad % 64 == 0 and one input view; x3q exists in fp32x3 only; the backward of mode fp32h is fp32x3's.  x3r at small
launches has 4 x 16 tiles only where Gh > 4 (xr_tile_height), so "exactly one tile" of that height does not exist: 8 x 16 is two of them,
4 x 16 is half a full-height tile; full 8 x 16 tiles and the <2, 1> form need more than 160 workgroups (the B = 32 cases).

Not covered here:
  - the fused dense-block kernels rdb_fwd.hip and rdb_tile.hip: their intermediate activations pass through fl(0.2f v) and a bf16 store, so
    a chain of five stages leaves every lattice.  tests/test_gpu_rdb_exact.py (over tests/rdb_lattice.py) holds them to exact sums one
    stage at a time - the stages before the one under test hand over lattice values - and to float64 stage by stage on normal data;
  - conv_x3c (opt-in, held bit-identical to four launches by tests/test_gpu_conv_x3.py);
  - ssr_conv2d_fixup."""
import pytest
import torch

import conv_lattice as cl

pytestmark = pytest.mark.gpu


def _name(c):
    return c.name


def check(case, data=None):
    res = cl.run(case, data)
    assert res.symbol.startswith(cl.symbol_prefix(case.family, case.mode)), f"{case.name}: forced {case.family}, launched {res.symbol}"
    msg = cl.mismatch(case, res, data)
    assert msg is None, msg
    return res


# ================================================================================================ fp16 specifics (the first fp32h cases)
@pytest.mark.parametrize("case", cl.F16_SINGLE, ids=_name)
def test_fp16_single_product(case):
    """one chunk, one non-zero channel, a 1 x 1 grid: every output is ONE product xh wh + xh wl + xl wh.  A failure here and not below
    would say that v_mfma_f32_32x32x16_f16 does not sum lattice products exactly, not that a kernel drops a term."""
    data = cl.single_product_data(case)
    x, w = data["x"][0, 0, 0, 0].double(), data["w"][:, 0, 1, 1].double()
    assert torch.equal(cl.expected(case, data)[0]["y"][0, 0, 0, 0].double(), x * w - (x - x.half().double()) * (w - (w * 1024).half().double() / 1024))
    check(case, data)


@pytest.mark.parametrize("case", cl.F16_SUBNORMAL, ids=_name)
def test_fp16_subnormal_lo_pieces(case):
    """x = +-1 + b 2^-16: the lo piece is an fp16 subnormal, which the converters and the matrix core must keep (a path that flushes it
    gives another sum)"""
    data = cl.subnormal_lo_data(case)
    lo = cl.half_planes(data["x"][..., :case.cin])[1]
    assert float(lo.abs().max()) == 2.0 ** -16 and float(lo.abs().max()) < 2.0 ** -14
    flushed = dict(data, x=cl.half_planes(data["x"])[0])
    assert not torch.equal(cl.expected(case, flushed)[0]["y"], cl.expected(case, data)[0]["y"]), "flushing the lo pieces must show"
    check(case, data)


# ================================================================================================ the families
@pytest.mark.parametrize("case", cl.GPU_CASES["x3r"], ids=_name)
def test_register_tiled(case):
    """csrc/conv_x3r.hip in split-bf16, exact fp32 and split-fp16: 1 .. 17 chunks against the eight-stage ring and the four K quarters
    (one chunk: fewer items than waves), masked channel tails, both tile heights, the 64-channel layer as two workgroups, two views"""
    res = check(case)
    ntw, nu, ep, th, am = (int(v) for v in res.symbol[res.symbol.index("<") + 1:-1].split(","))
    gh, gw = case.out_hw
    # xr_tile_height / xr_wide_form (csrc/conv_x3r.hip:557-580): at most 160 workgroups -> 4 x 16 tiles, two workgroups per 64 channels
    assert (ntw, nu) == (1, 1) and th == (4 if gh > 4 else 8) and am == {"fp32x3": 0, "fp32": 1, "fp32h": 2}[case.mode]


@pytest.mark.parametrize("case", cl.GPU_CASES["forms"], ids=_name)
def test_forms_that_only_the_launch_size_selects(case):
    """B = 32 at 32 x 32: x3r's full-height tiles <1, 1, ., 8, .> and its <2, 1> form, the 8 x 16 tile (four waves) of the pipelined kernel"""
    res = check(case)
    if case.family == "x3r":
        assert res.symbol.startswith("conv_x3r_kernel<2, 1, " if case.cout == 64 else "conv_x3r_kernel<1, 1, ") and ", 8, " in res.symbol
    else:
        assert res.symbol.endswith("W4>"), res.symbol


@pytest.mark.parametrize("case", cl.GPU_CASES["x3q"], ids=_name)
def test_ring(case):
    """csrc/conv_x3q.hip (the family the library never picks by itself)"""
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["pipelined"], ids=_name)
def test_pipelined(case):
    """conv_kernel / conv_x3_kernel / conv_h3_kernel of csrc/conv.hip in all four modes, the ReLU epilogues and the kernel's own 4x4
    stride-2 form (a layer kept off the space-to-depth path) included"""
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["res"], ids=_name)
def test_k_resident(case):
    """csrc/conv_res.hip (bf16, exact fp32): reached as `every family that cannot be forced`, proven by the symbol"""
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["thin"], ids=_name)
def test_thin_output(case):
    """csrc/conv_thin.hip: 1, 3, 5 and 8 output channels; in the split modes w = hi + lo is rebuilt in fp32: the full product"""
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["bigx3"], ids=_name)
def test_big_tile_split(case):
    """conv_bigx3_kernel4 / conv_bigh3_kernel4 <3> and <2> (space-to-depth forward): persistent over images with one and two image groups,
    single-buffer 16-channel chunks, the nearest x2 read; bigh3 starts its accumulators at 2^10 bias"""
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["big"], ids=_name)
def test_big_tile_bf16(case):
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["ws"], ids=_name)
def test_weight_stationary(case):
    check(case)


@pytest.mark.parametrize("case", cl.GPU_CASES["parity-classes"], ids=_name)
def test_stride2_dgrad_parity_classes(case):
    """the four 2 x 2 classes of a 4x4 stride-2 data gradient through ssr_conv2d_batch, each writing every second row and column of y: in
    one big-tile launch (conv_bigx3_kernel4<2>, conv_big_kernel4; SSR_X3_BIGTILE2 / SSR_CONV_BIGTILE2 = 2) and as the library deals them at
    this size (bf16: conv_kernel4, one pipelined launch; fp32 modes: four).  ssr_conv2d_batch takes no impl and reports no symbol: the
    one asserted is ssr_conv2d_symbol of a class where the library deals them itself, and where the switch forces the big tile only
    select's answer that the family can run the class - the switch is what sends the batch there (ssr_conv_*_batch_try), not proven here"""
    check(case)


# ================================================================================================ properties across cases
BATCH_LEGS = [next(c for c in cases if c.B == 3 and c.kind == "k3" and c.mode == mode and (c.H, c.W) in ((9, 17), (33, 17), (9, 33)))
              for fam, cases in cl.GPU_CASES.items() if fam in cl.MODES_OF for mode in cl.MODES_OF[fam]]


@pytest.mark.parametrize("case", BATCH_LEGS, ids=_name)
def test_bytes_of_an_image_do_not_depend_on_the_batch(case):
    """image 0 alone and as the first of three: free once both are exact, asserted all the same"""
    from dataclasses import replace
    three, one = check(case), check(replace(case, B=1))
    for name in ("y", "y0", "y1"):
        a, b = getattr(one, name), getattr(three, name)
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), name


SEEN = [next(c for c in cl.GPU_CASES[fam] if c.mode == mode and c.kind == "k3" and (c.H, c.W) == cl.MID and c.variant == "lrelu")
        for fam, mode in (("x3r", "fp32x3"), ("x3r", "fp32h"), ("bigx3", "fp32x3"), ("bigx3", "fp32h"), ("pipelined", "fp32h"), ("x3q", "fp32x3"))]


@pytest.mark.parametrize("case", SEEN, ids=_name)
def test_one_step_of_one_lo_piece_is_seen(case):
    """the control of this file: ONE input element moved by one lattice step (its lo piece only) changes exactly the outputs it reaches,
    on the device as in the float64 sum, and fails against the expectation of the unmoved input"""
    data = {k: v.clone() for k, v in cl.inputs(case).items()}
    step = 2.0 ** -cl.GRANULE_BITS[cl.arithmetic(case.family, case.mode)[0]]
    x = data["x"][0, 4, 8, 5].clone()
    hi = float(cl.term_pairs(x.double(), x.double(), cl.arithmetic(case.family, case.mode)[1])[0][0])
    data["x"][0, 4, 8, 5] = hi + (step if float(x) <= hi else 0.0)                              # lo: 0 or -step -> +step; +step -> 0
    assert float(data["x"][0, 4, 8, 5]) != float(x)
    res = check(case, data)
    far = cl.mismatch(case, res)
    assert far is not None and "y:" in far, "the moved lo piece must fail against the unmoved expectation"
    moved = res.y != cl.run(case).y
    assert bool(moved.any()) and not bool(moved[1:].any()) and not bool(moved[0, :3].any()) and not bool(moved[0, 6:].any())
