"""CPU: tests/conv_lattice.py itself - the float64 contract reference against explicit loops and F.unfold for every kind of layer, the
lattices and their bf16 / fp16 pieces (the 2^10 weight shift included) under torch's own conversions, the exactness condition of EVERY
case tests/test_gpu_conv_exact.py runs (the shared lists), that the expected bits move under a dropped, a doubled, a shifted product, a
dropped lo.hi term and an added lo.lo term, and the candidate rule of the generic epilogue against numpy fp32 evaluations.
Run with -s to see the largest exactness margin (kept in profiles/conv_exact/exactness_margins.txt)."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_lattice as cl


# ================================================================================================ the reference
def loop_reference(x, w, kind, up=1):
    """y[n, co, gy, gx] = sum x[n, ci, (gy s + ky - pad) // up, (gx s + kx - pad) // up] w[co, ci, ky, kx] as include/ssr_hip.h states it;
    the data gradients as the scatter of every input pixel into the outputs it reaches (weights [ci, co, ky, kx])"""
    k, s = cl.KINDS[kind]
    B, ci, H, W = x.shape
    if kind in ("k3", "s2d", "k4"):
        gh, gw = (H * up, W * up) if kind == "k3" else (H // 2, W // 2)
        y = torch.zeros(B, w.shape[0], gh, gw, dtype=torch.float64)
        for gy, gx, ky, kx in itertools.product(range(gh), range(gw), range(k), range(k)):
            iy, ix = gy * s + ky - 1, gx * s + kx - 1
            if 0 <= iy < H * up and 0 <= ix < W * up:
                y[:, :, gy, gx] += x[:, :, iy // up, ix // up] @ w[:, :, ky, kx].T
        return y
    gh, gw = H * s, W * s
    y = torch.zeros(B, w.shape[1], gh, gw, dtype=torch.float64)
    for iy, ix, ky, kx in itertools.product(range(H), range(W), range(k), range(k)):
        oy, ox = iy * s + ky - 1, ix * s + kx - 1
        if 0 <= oy < gh and 0 <= ox < gw:
            y[:, :, oy, ox] += x[:, :, iy, ix] @ w[:, :, ky, kx]
    return y


def unfold_reference(x, w, kind, up=1):
    """forward kinds: patches by F.unfold and one matrix product.  dgrad4 in the form the device runs it: four 2 x 2 stride-1 convolutions,
    class (py, px) with pad (1 - py, 1 - px) over taps ky = 3 - py - 2 dy, written to every second row and column (engine._ConvBuilder.dgrad,
    misc.hip's packing); dgrad3 as the forward conv with the weights rotated by 180 degrees and transposed"""
    k, s = cl.KINDS[kind]
    if kind in ("k3", "s2d", "k4"):
        if up == 2:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        cols = F.unfold(x, k, padding=1, stride=s)
        gh, gw = (x.shape[2], x.shape[3]) if kind == "k3" else (x.shape[2] // 2, x.shape[3] // 2)      # (odd sizes: the last row has no output)
        return torch.einsum("ok,bkp->bop", w.flatten(1), cols).view(x.shape[0], w.shape[0], gh, gw)
    if kind in ("dgrad3", "gather"):
        return unfold_reference(x, w.flip(2, 3).transpose(0, 1), "k3")
    B, _, H, W = x.shape
    y = torch.zeros(B, w.shape[1], 2 * H, 2 * W, dtype=torch.float64)
    for py, px in itertools.product((0, 1), (0, 1)):
        wc = torch.stack([torch.stack([w[:, :, 3 - py - 2 * dy, 3 - px - 2 * dx] for dx in (0, 1)], -1) for dy in (0, 1)], -2)   # [ci, co, 2, 2]
        xp = F.pad(x, (1 - px, px, 1 - py, py))
        y[:, :, py::2, px::2] = F.conv2d(xp, wc.transpose(0, 1))
    return y


SMALL = [("k4", 2, 5, 6, 3, 2, 1), ("k4", 1, 2, 2, 2, 3, 1), ("k3", 2, 4, 3, 5, 3, 1), ("k3", 1, 1, 1, 3, 2, 1), ("k3", 2, 3, 5, 2, 3, 2), ("k3", 1, 1, 2, 3, 2, 2),
         ("s2d", 2, 4, 6, 3, 2, 1), ("s2d", 1, 2, 2, 2, 3, 1), ("dgrad3", 2, 4, 3, 3, 2, 1), ("dgrad3", 1, 1, 1, 2, 3, 1),
         ("dgrad4", 2, 3, 2, 3, 2, 1), ("dgrad4", 1, 1, 1, 2, 3, 1)]


@pytest.mark.parametrize("kind,B,H,W,ci,co,up", SMALL, ids=[f"{s[0]}-{s[1]}x{s[2]}x{s[3]}-up{s[6]}" for s in SMALL])
@pytest.mark.parametrize("lattice", ["coarse", "split", "half", "randn"])
def test_reference_agrees_with_explicit_loops_and_with_unfold(kind, B, H, W, ci, co, up, lattice):
    case = cl.Case("pipelined", "fp32", kind, B, H, W, ci, co, up=up)
    gen = (lambda shape, seed: torch.randn(shape, generator=torch.Generator().manual_seed(seed))) if lattice == "randn" else cl.LATTICES[lattice]
    x, w = gen((B, ci, H, W), 1).double(), gen(cl.weight_shape(case), 2).double()
    y = cl.contract(x, w, kind, up)
    assert tuple(y.shape) == (B, co) + case.out_hw
    for other in (loop_reference, unfold_reference):
        o = other(x, w, kind, up)
        if lattice == "randn":                    # float64 sums in another order
            assert float((y - o).abs().max()) < 1e-12 * float(y.abs().max())
        else:                                     # exact sums: equal whatever the order
            assert torch.equal(y, o), other.__name__


@pytest.mark.parametrize("c1", [16, 32])
def test_two_views_are_the_channel_concatenation(c1):
    """[x | x2] against one weight = the sum of the two partial convolutions (include/ssr_hip.h, ssr_conv_desc.x2)"""
    case = cl.Case("x3r", "fp32x3", "k3", 2, 5, 4, 48, 8, "mask", c1=c1)
    d = cl.inputs(case)
    x, w = d["x"].double().permute(0, 3, 1, 2), d["w"].double()
    whole = cl.contract(x, w, "k3")
    assert torch.equal(whole, cl.contract(x[:, :c1], w[:, :c1], "k3") + cl.contract(x[:, c1:], w[:, c1:], "k3"))


# ================================================================================================ the lattices
def test_half_lattice_and_its_fp16_pieces():
    h = cl.half_lattice((4, 33, 17, 24), 3)
    a = h.round()
    assert set(torch.unique(a.abs()).tolist()) == {2.0, 3.0}
    assert set(torch.unique((h.double() - a.double()) * 4096).tolist()) == {-1.0, 0.0, 1.0}, "a + b * 2^-12, exact in fp32"
    assert torch.equal(h.to(torch.float16).float(), a), "f16(x) == a"
    assert torch.equal((h * 1024).to(torch.float16).float(), a * 1024), "f16(2^10 w) == 2^10 a"
    hi, lo = cl.half_planes(h)
    assert torch.equal(hi, a) and torch.equal(lo.double(), h.double() - a.double()) and torch.equal(hi + lo, h)
    whi, wlo = cl.half_planes(h, cl.WSHIFT)
    assert torch.equal(whi, hi) and torch.equal(wlo, lo), "the weight pieces are those of 2^10 w and the 2^-10 comes back exactly"
    assert set(torch.unique(((h * 1024) - (h * 1024).to(torch.float16).float())).tolist()) == {-0.25, 0.0, 0.25}
    # no round-to-even tie: the distance to the fp16 neighbours of a is never half a unit in the last place (2^-9 / 2 at [2, 4); 2^-10 / 2
    # just below 2): a - 2^-12 is a quarter unit below a = 2, an eighth elsewhere.  a = 1 would tie: 1 - 2^-12 is half way to 1 - 2^-11.
    for v in (2.0 - 2.0 ** -12, 2.0 + 2.0 ** -12, 3.0 - 2.0 ** -12, 3.0 + 2.0 ** -12):
        unit_below = float(np.spacing(np.float16(v - 0.01)))                  # (2^-10 just below 2, 2^-9 above)
        assert abs(float(np.float16(v)) - v) == 2.0 ** -12 < unit_below / 2
        assert abs(float(np.float16(1024 * v)) - 1024 * v) == 0.25 < float(np.spacing(np.float16(1024 * (v - 0.01)))) / 2
    assert float(np.spacing(np.float16(0.9))) / 2 == 2.0 ** -12, "the tie that a = +-1 would meet"
    assert float((lo != 0).float().mean()) > 0.5


def test_split_lattice_pieces_and_what_the_modes_multiply():
    s = cl.split_lattice((3, 9, 17, 16), 5)
    (xh, xl), (wh, wl) = cl.split_planes(s), cl.split_planes(s.flip(0))
    pairs = cl.term_pairs(s.double(), s.flip(0).double(), "bf16")
    assert len(pairs) == 3 and torch.equal(pairs[0][0], xh.double()) and torch.equal(pairs[1][1], wl.double()) and torch.equal(pairs[2][0], xl.double())
    assert torch.equal(pairs[2][1], wh.double()), "xh wh + xh wl + xl wh: lo.lo is not among them"
    h = cl.half_lattice((3, 9, 17, 16), 6)
    pairs = cl.term_pairs(h.double(), h.flip(0).double(), "f16")
    total = sum(a * b for a, b in pairs)
    lo_lo = cl.half_planes(h)[1].double() * cl.half_planes(h.flip(0), cl.WSHIFT)[1].double()
    assert torch.equal(total + lo_lo, h.double() * h.flip(0).double())
    assert len(cl.term_pairs(s.double(), s.double(), None)) == 1
    # thin<., 1 | 2>: w on the mode's lattice, lo plane not empty, hi + lo = w in fp32; x integer
    for mode, planes in (("fp32x3", cl.split_planes), ("fp32h", lambda t: cl.half_planes(t, cl.WSHIFT))):
        case = cl.Case("thin", mode, "k3", 1, 9, 17, 24, 5)
        d = cl.inputs(case)
        hi, lo = planes(d["w"])
        assert cl.arithmetic("thin", mode)[1] is None and float((lo != 0).float().mean()) > 0.5 and torch.equal(hi + lo, d["w"])
        assert torch.equal(d["x"], d["x"].round()) and float(d["x"][..., :24].abs().min()) >= 1
    assert cl.arithmetic("thin", "fp32") == cl.arithmetic("thin", "bf16") == ("coarse", None)


def test_inputs_share_images_between_batch_sizes_and_zero_the_view_padding():
    a, b = cl.Case("x3r", "fp32", "k3", 1, 9, 17, 5, 32, cin_view=8), cl.Case("x3q", "fp32", "k3", 3, 9, 17, 5, 32, cin_view=8)
    da, db = cl.inputs(a), cl.inputs(b)
    for k in ("x", "r1", "r2", "yold", "m"):
        assert torch.equal(da[k][0], db[k][0])
    assert torch.equal(da["w"], db["w"]) and da["x"].shape[-1] == 8 and float(da["x"][..., 5:].abs().max()) == 0 and float(da["x"][..., :5].abs().min()) > 0
    m = cl.inputs(cl.ALL_CASES[0])["m"]
    assert bool((m == 0).any()) and bool((m > 0).any()) and bool((m < 0).any()), "exact zeros and both signs in the mask"
    w = cl.inputs(next(c for c in cl.ALL_CASES if c.mode == "fp32h" and c.K == 1728 and c.family == "x3r"))["w"]
    assert 0.1 < float((w != 0).float().mean()) < 0.2, "fp32h at K = 1728: thinned weights, the full contraction"


def test_every_epilogue_constant_is_a_power_of_two():
    for name, ep in cl.EPILOGUES.items():
        for v in (ep.alpha, ep.r1, ep.r2):
            assert v is None or float(np.log2(abs(v))).is_integer(), name
    assert {ep.alpha < 0 or (ep.r1 or 1) < 0 or (ep.r2 or 1) < 0 for ep in cl.EPILOGUES.values()} == {True, False}, "either sign"


# ================================================================================================ exactness of every GPU case
def test_exactness_condition_and_fp32_exact_targets_of_every_case():
    """`expected` asserts sum |terms| < 2^24 granules per output element, that the pre-activation is an fp32 number and that every element
    without a rounding on its path has ONE target, the float64 value"""
    assert len(set(cl.ALL_CASES)) == len(cl.ALL_CASES) > 900
    worst = (0.0, None)
    for case in cl.ALL_CASES:
        exp, margin = cl.expected(case)
        assert 0 < margin < 1
        Ho, Wo = case.out_hw
        assert exp["y"].shape[1:] == (case.B, Ho, Wo, case.cout) and bool(torch.isfinite(exp["y"]).all())
        worst = max(worst, (margin, case.name))
    for case, make in [(c, cl.single_product_data) for c in cl.F16_SINGLE] + [(c, cl.subnormal_lo_data) for c in cl.F16_SUBNORMAL]:
        worst = max(worst, (cl.expected(case, make(case))[1], case.name))
    print(f"\nlargest margin: {worst[0]:.4f} of 2^24 granules ({worst[1]})", end="")
    # K = 1728 (192 channels, 3x3) is a case of every family that runs it, in every mode
    for fam in ("x3r", "x3q", "pipelined", "bigx3", "big"):
        for mode in cl.MODES_OF[fam]:
            assert any(c.K == 1728 for c in cl.GPU_CASES[fam] if c.mode == mode), (fam, mode)
    assert any(c.K == 1728 and c.mode == "bf16" for c in cl.GPU_CASES["res"])


def test_exactness_condition_rejects_a_sum_that_is_too_long():
    """the condition is live: the half lattice WITHOUT thinning breaks it at K = 1728"""
    case = next(c for c in cl.ALL_CASES if c.mode == "fp32h" and c.K == 1728 and c.family == "x3r")
    data = dict(cl.inputs(case), w=cl.half_lattice(cl.weight_shape(case), 9))
    with pytest.raises(AssertionError, match="not exact in every order"):
        cl.expected(case, data)


def test_res_cases_fit_the_kernel():
    assert all(cl.res_fits(c) for c in cl.GPU_CASES["res"])
    assert not cl.res_fits(cl.Case("res", "fp32", "k3", 1, 9, 17, 128, 32)) and cl.res_fits(cl.Case("res", "bf16", "k3", 1, 9, 17, 192, 64))


# ================================================================================================ sensitivity
def _one_per_family_and_arithmetic():
    seen = {}
    for c in cl.ALL_CASES:
        if (c.H, c.W) == cl.MID or c.kind in ("s2d", "k4", "dgrad4"):
            seen.setdefault((c.family, c.mode, c.kind), c)
    return list(seen.values())


@pytest.mark.parametrize("case", _one_per_family_and_arithmetic(), ids=lambda c: c.name)
def test_expected_bits_move_under_every_mutation(case):
    """one product dropped, doubled, read one column off; one lo.hi term dropped; the lo.lo term added: each changes the expected bits of
    at least one element (of exactly the elements it reaches where that is one product), through the epilogue, in the stored format"""
    data = cl.inputs(case)
    pieces = cl.arithmetic(case.family, case.mode)[1]
    pre, _ = cl.accumulate(case, data)
    bf16 = case.mode == "bf16"
    base = cl.finish(pre, case.ep, data, bf16)["y"]
    x, w = data["x"][..., :case.cin].double().permute(0, 3, 1, 2), data["w"].double()
    n, ci = case.B - 1, case.cin - 1
    iy, ix = case.H // 2, min(case.W - 2, case.W // 2)

    def delta(xs, ws):
        """the contribution of input element (n, ci, iy, ix) of `xs` against `ws` to every output"""
        one = torch.zeros_like(x)
        one[n, ci, iy, ix] = xs[n, ci, iy, ix]
        return cl.contract(one, ws, case.kind, case.up)

    def moved(pre2):
        out = cl.finish(pre2, case.ep, data, bf16)["y"]
        return ~((out.unsqueeze(1) == base.unsqueeze(0)).any(0).all(0))       # no candidate of the mutation is a candidate of the truth

    full = sum(delta(a, b) for a, b in cl.term_pairs(x, w, pieces))
    reach = (full != 0).permute(0, 2, 3, 1)
    assert bool(reach.any())
    for what, pre2 in (("dropped", pre - full), ("doubled", pre + full)):
        mv = moved(pre2)
        assert bool(mv.any()) and not bool(mv[~reach].any()), what
        # fp32 storage: exactly the outputs the element reaches change.  bf16 storage keeps 8 bits: one product (at most 9.4) against a
        # sum near 128 can stay below half a unit of the stored value in SOME of them - a property of the format, not of the test
        assert bf16 or torch.equal(mv, reach), f"{what}: exactly the outputs the element reaches change"
    xs = x.clone()
    xs[n, ci, iy, ix] = x[n, ci, iy, ix + 1] if float(x[n, ci, iy, ix + 1]) != float(x[n, ci, iy, ix]) else -x[n, ci, iy, ix]
    shifted = sum(delta(a, b) for a, b in cl.term_pairs(xs, w, pieces))
    assert bool(moved(pre - full + shifted).any()), "a misplaced tap is a different number"
    if pieces:
        (xh, wh), (_, wl), (xl, _) = cl.term_pairs(x, w, pieces)
        xl = xl.clone()
        if float(xl[n, ci, iy, ix]) == 0:                                    # (b = 0 at this element: another element of the pixel)
            ci = int((xl[n, :, iy, ix] != 0).nonzero()[0])
        assert bool(moved(pre - delta(xl, wh)).any()), "one lo.hi term of one chunk dropped"
        assert bool(moved(pre - delta(xh, wl)).any()) or float(wl.abs().max()) == 0, "one hi.lo term dropped"
        lolo = cl.contract(xl, wl, case.kind, case.up)
        # (bf16 pieces: multiples of 2^-18; fp16 pieces: of 2^-24, at most K 2^-24 - seen wherever the sum is small enough for its fp32 unit)
        assert bool(moved(cl.r32(pre + lolo)).any()), "the lo.lo term added (four products instead of three)"


# ================================================================================================ the candidate rule
def test_ordered_partitions():
    assert [len(cl.ordered_partitions("abcd"[:n])) for n in range(5)] == [1, 1, 3, 13, 75]
    parts = cl.ordered_partitions("abc")
    assert len({tuple(tuple(sorted(b)) for b in p) for p in parts}) == 13 and all(sorted(sum(p, [])) == list("abc") for p in parts)


def test_candidate_rule_accepts_every_grouped_fp32_evaluation_and_nothing_else():
    """the generic epilogue after a negative LeakyReLU: s0 = alpha fl(0.2f v), then beta1 r1, beta2 r2 and y_old in any grouped order, each
    step one numpy fp32 operation; then the mask"""
    case = cl.Case("x3r", "fp32x3", "k3", 2, 9, 17, 96, 32, "generic")
    data = cl.inputs(case)
    exp, _ = cl.expected(case)
    ep = case.ep
    pre = cl.accumulate(case, data)[0].permute(0, 2, 3, 1).numpy()
    f = np.float32
    v = pre.astype(f)
    s0 = np.where(v > 0, v, f(0.2) * v) * f(ep.alpha)
    assert exp["y0"].shape[0] == 1 and np.array_equal(exp["y0"][0].numpy(), s0)
    t = {"r1": f(ep.r1) * data["r1"].numpy(), "r2": f(ep.r2) * data["r2"].numpy(), "yold": data["yold"].numpy()}
    m = data["m"].numpy()
    seen = set()
    for part in cl.ordered_partitions(t):
        a = s0
        for block in part:
            g = t[block[0]]
            for k in block[1:]:
                g = g + t[k]                          # (sums of lattice values: exact in fp32)
            a = a + g
        assert a.dtype == np.float32
        y = np.where(m > 0, a, a * f(0.2))
        assert bool(cl.member(torch.from_numpy(a), exp["y1"]).all()) and bool(cl.member(torch.from_numpy(y), exp["y"]).all())
        seen.add(a.tobytes())
    assert len(seen) > 1, "the orders do differ somewhere"
    # the left-to-right order of conv_epilogue.h, v += (beta1 r1 + beta2 r2) + y_old, is one of them
    a = s0 + ((t["r1"] + t["r2"]) + t["yold"])
    assert bool(cl.member(torch.from_numpy(a), exp["y1"]).all())
    # one unit in the last place off every candidate: rejected, on rounded and on exact elements alike
    y1 = exp["y1"]
    for off in (np.nextafter(y1.max(0).values.numpy(), f(np.inf)), np.nextafter(y1.min(0).values.numpy(), f(-np.inf))):
        assert not bool(cl.member(torch.from_numpy(off), y1).any())
    many = (y1 != y1[:1]).any(0)
    rounded = torch.from_numpy(pre < 0)
    assert bool(many.any()) and not bool(many[~rounded].any()), "more than one target only where a rounded value is followed by several terms"
    assert not bool(cl.member(torch.full_like(y1[0], float("nan")), y1).any())


def test_one_further_term_after_a_rounding_has_a_single_target():
    case = cl.Case("x3r", "fp32x3", "k3", 1, 9, 17, 96, 32, "lrelu_r1_y0")
    exp, _ = cl.expected(case)
    assert exp["y"].shape[0] == 1 and exp["y1"].shape[0] == 1
    bf = cl.expected(cl.Case("pipelined", "bf16", "k3", 1, 9, 17, 96, 32, "lrelu_r1_y0"))[0]["y"]
    assert torch.equal(bf.bfloat16().float(), bf), "bf16 storage: the fp32 result rounded once more"
