"""CPU: tests/wgrad_lattice.py itself - the float64 reference against an independent formulation, the lattices' representability, the
exactness condition and fp32-exact expected values for EVERY case tests/test_gpu_wgrad_exact.py runs (the shared list ALL_CASES), that
the three-term expectation of the fp32x3 forms is distinguishable from the full product, and that the expected bits move when one
pixel's term is dropped, one tap is shifted by one or one term is added twice (no blind spot through cancellation at these shapes).
Run with -s to see the exactness margin of every case (kept in profiles/wgrad_exact/README.md)."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_lattice as wl


def _ids(cases):
    return [f"{c.name}-{lat}{'-x' + str(n) if n > 1 else ''}{'-prefilled' if pre else ''}" for c, lat, n, pre in cases]


# ================================================================================================ the reference
def unfold_reference(x, dy, kind, up=1):
    """the same sums without autograd and without conv2d: patches by F.unfold, one einsum over (image, pixel)"""
    k, s, pad = wl.KINDS[kind]
    if up == 2:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    cols = F.unfold(x, k, padding=pad, stride=s)                                     # [B, Cin * k * k, pixels]
    dyf = dy.flatten(2)                                                              # [B, Cout, pixels]
    return torch.einsum("bop,bcp->oc", dyf, cols).view(dy.shape[1], x.shape[1], k, k), dyf.sum(dim=(0, 2))


def loop_reference(x, dy, kind, up=1):
    """dW[co][ci][ky][kx] = sum dY[n, gy, gx, co] * X[n, gy * stride + ky - pad, gx * stride + kx - pad, ci], as include/ssr_hip.h states it"""
    k, s, pad = wl.KINDS[kind]
    B, co, gh, gw = dy.shape
    lh, lw = x.shape[2] * up, x.shape[3] * up
    dw = torch.zeros(co, x.shape[1], k, k, dtype=torch.float64)
    for n in range(B):
        for gy in range(gh):
            for gx in range(gw):
                for ky in range(k):
                    for kx in range(k):
                        iy, ix = gy * s + ky - pad, gx * s + kx - pad
                        if 0 <= iy < lh and 0 <= ix < lw:
                            dw[:, :, ky, kx] += torch.outer(dy[n, :, gy, gx], x[n, :, iy // up, ix // up])
    return dw, dy.sum(dim=(0, 2, 3))


SMALL = [wl.k3_case("small-up2", 2, (6, 10), ((5, 3),), up=2), wl.k3_case("small-p0", 2, (3, 5), ((4, 6),), pad=0),
         wl.k4_case("small-k4-odd", 2, (5, 8), ((3, 4),)), wl.k3_case("small-k3", 1, (4, 3), ((2, 2),))]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
@pytest.mark.parametrize("lattice", ["coarse", "split", "randn"])
def test_reference_agrees_with_unfold_and_with_explicit_loops(case, lattice):
    x, dy = wl.layer_operands(case, wl.inputs(case, lattice), 0)
    assert tuple(dy.shape[2:]) == case.grid
    dw, db = wl.wgrad_reference(x, dy, case.kind, case.up)
    for other in (unfold_reference, loop_reference):
        ow, ob = other(x, dy, case.kind, case.up)
        if lattice == "randn":                    # float64 sums in another order: a few ulps of the largest partial sum
            assert float((dw - ow).abs().max()) < 1e-12 * float(dw.abs().max()) and float((db - ob).abs().max()) < 1e-12 * float(db.abs().max())
        else:                                     # exact sums: equal whatever the order
            assert torch.equal(dw, ow) and torch.equal(db, ob)


# ================================================================================================ the lattices
def test_lattice_values_are_exact_in_their_formats():
    c = wl.coarse_lattice((4, 33, 17, 24), 1)
    assert torch.equal(c.to(torch.bfloat16).float(), c), "the coarse lattice is exactly bf16"
    assert set(torch.unique((c * 16).round().abs() // 16).tolist()) <= {0.0, 1.0, 2.0, 3.0} and float(c.abs().min()) >= 15 / 16
    assert torch.unique(c).numel() == 18          # +-{1, 2, 3} + {-1, 0, 1} / 16
    s = wl.split_lattice((4, 33, 17, 24), 2)
    a = s.round()
    assert torch.equal((a.double() + (s.double() - a.double())).float(), s)
    assert set(torch.unique(a.abs()).tolist()) == {1.0, 2.0, 3.0}
    assert set(torch.unique((s.double() - a.double()) * 512).tolist()) == {-1.0, 0.0, 1.0}, "a + b * 2^-9, exact in fp32"
    hi, lo = wl.split_planes(s)
    assert torch.equal(hi, a), "ssr_split_bf16's hi plane is the integer part (1 - 2^-9 is a tie that rounds to even: 1)"
    assert torch.equal(hi + lo, s) and torch.equal(hi.double() + lo.double(), s.double())
    assert float((lo != 0).float().mean()) > 0.5 and set(torch.unique(lo * 512).tolist()) == {-1.0, 0.0, 1.0}
    # two generators, two streams
    assert not torch.equal(wl.coarse_lattice((64,), 1), wl.coarse_lattice((64,), 2))
    assert torch.equal(wl.coarse_lattice((64,), 1), wl.coarse_lattice((64,), 1))


def test_buffers_hold_nan_outside_the_views_and_zero_in_their_padding():
    case = wl.DENSE_FIRST
    data = wl.inputs(case, "coarse")
    assert data["x"].shape == (2, 13, 21, 192) and data["g"].shape == (2, 13, 21, 192)
    assert bool(torch.isfinite(data["x"][..., :64]).all()) and bool(torch.isnan(data["x"][..., 64:]).all())
    assert bool(torch.isnan(data["g"][..., :64]).all()) and bool(torch.isfinite(data["g"][..., 64:96]).all())
    assert bool(torch.isnan(data["g"][..., 96:]).all())
    case = wl.CHANNEL_K3[0]                       # 3 -> 64 in a 8-channel view
    x = wl.inputs(case, "coarse")["x"]
    assert x.shape[-1] == 8 and float(x[..., :3].abs().min()) > 0 and float(x[..., 3:].abs().max()) == 0
    case = wl.CHANNEL_K3[2]                       # 64 -> 1: seven zero channels of dY, a 72-channel view of x
    assert wl.inputs(case, "coarse")["x"].shape[-1] == 72
    dy = wl.inputs(case, "coarse")["dy0"]
    assert dy.shape[-1] == 8 and float(dy[..., 1:].abs().max()) == 0
    dense = wl.inputs(wl.DENSE_CASES[0], "split")
    assert bool(torch.isfinite(dense["x"]).all()) and bool(torch.isnan(dense["g"][..., :64]).all()) and bool(torch.isfinite(dense["g"][..., 64:]).all())


def test_tile_cases_cut_into_the_ranges_they_are_meant_to():
    """the even ranges WgradBatch.add cuts (wgrad_plan.cut: per = ceil(tiles / ceil(tiles / cap))) are the cap itself for 1, NST,
    NST + 1 and 2 NST + 1, and none of them lines up with the images"""
    for (mode, kind), (case, th, (ty, tx)) in wl.TILE_CASES.items():
        gh, gw = case.grid
        assert (-(-gh // th), -(-gw // 16)) == (ty, tx) and case.kind == kind, (mode, kind, case.grid)
        assert gh % th and gw % 16, "ragged in both directions"
        assert th == wl.tile_rows(mode, kind)
        nst, tiles = wl.ring_stages(mode, kind), case.B * ty * tx
        assert nst == (3 if (mode in ("bf16", "x3pass") and kind == "k4") else 2)
        for cap in (1, nst, nst + 1, 2 * nst + 1):
            per = -(-tiles // -(-tiles // cap))
            assert per == cap and cap % (ty * tx), (mode, kind, cap, per)
            assert any(b % (ty * tx) for b in range(0, tiles, per)), "some range begins inside an image"


# ================================================================================================ exactness of every GPU case
@pytest.mark.parametrize("case,lattice,launches,prefilled", wl.ALL_CASES, ids=_ids(wl.ALL_CASES))
def test_exactness_condition_and_fp32_exact_expected_values(case, lattice, launches, prefilled):
    """`expected` asserts sum |terms| * 2^g < 2^24 per output element and that the float64 value is an fp32 number"""
    assert case.pixels <= 4096
    exp, margin = wl.expected(case, lattice, lattice == "split", launches, prefilled)
    assert 0 < margin < 1 and len(exp) == len(case.layers)
    for (dw, db), L in zip(exp, case.layers):
        assert dw.dtype == torch.float32 and bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        assert dw.shape == (L.cout, L.cin) + (wl.KINDS[case.kind][0],) * 2 and float(dw.abs().max()) > 0
    print("\n" + wl.margin_line(case, lattice, lattice == "split", launches, prefilled), end="")


def test_exactness_condition_rejects_a_sum_that_is_too_long():
    """the condition is live: at 16384 pixels (four times the 4096 the cases stay under) sum |terms| passes 2^24 granules.  (alpha cannot
    do that: it scales the terms and the granule alike.)"""
    case = wl.k3_case("too-long", 4, (64, 64), (wl.Layer(8, 8),))
    with pytest.raises(AssertionError, match="not exact in every order"):
        wl.expected(case, "split", True)


@pytest.mark.parametrize("case", [wl.DENSE_CASES[1], wl.CHANNEL_K3[3], wl.GRID_K4[3]], ids=lambda c: c.name)
def test_three_term_expectation_differs_from_the_full_product(case):
    """the dropped lo.lo term is visible: somewhere the two expectations are more than one fp32 ulp apart, so a kernel that formed four
    products (or two) could not pass for one that forms three"""
    three, full = wl.reference(case, "split", True), wl.reference(case, "split", False)
    for (tw, tb, _, _), (fw, fb, _, _) in zip(three, full):
        ulp = 2.0 ** (torch.floor(torch.log2(tw.abs().clamp_min(2.0 ** -126))) - 23)
        assert bool(((tw - fw).abs() > ulp).any())
        assert torch.equal(tb, fb), "the bias gradient has no dropped term: sum dy_hi + sum dy_lo = sum dy"
        assert float((tw - fw).abs().max()) < 2e-6 * float(fw.abs().max()), "the lo.lo term: about 2^-18 relative"


# ================================================================================================ sensitivity
_PERTURBED = sorted({(c, lat) for c, lat, n, pre in wl.ALL_CASES if n == 1 and not pre}, key=lambda e: (e[0].name, e[1]))


@pytest.mark.parametrize("case,lattice", _PERTURBED, ids=[f"{c.name}-{lat}" for c, lat in _PERTURBED])
def test_expected_bits_move_under_a_dropped_a_doubled_and_a_shifted_term(case, lattice):
    three = lattice == "split"
    k, s, pad = wl.KINDS[case.kind]
    data = wl.inputs(case, lattice)
    gh, gw = case.grid
    lh, lw = case.Hi * case.up, case.Wi * case.up
    n, gy, gx = case.B - 1, gh // 2, gw - 1                # a pixel of the last image, on the right edge of the grid
    inside = torch.tensor([[0 <= gy * s + ky - pad < lh and 0 <= gx * s + kx - pad < lw for kx in range(k)] for ky in range(k)])
    assert bool(inside.any())
    for i in sorted({0, len(case.layers) - 1}):
        x, dy = wl.layer_operands(case, data, i)
        ref_w, ref_b = (t.float() for t in wl.layer_reference(x, dy, case.kind, case.up, three)[:2])
        for factor in (0.0, 2.0):                          # one pixel's term dropped / added twice
            d2 = dy.clone()
            d2[n, :, gy, gx] *= factor
            w, b = (t.float() for t in wl.layer_reference(x, d2, case.kind, case.up, three)[:2])
            assert torch.equal(w != ref_w, inside.expand_as(w)), "exactly the taps that see the pixel change, for every (co, ci)"
            assert bool((b != ref_b).all())
        # tap (1, 1) - inside the image for at least one pixel of every grid here - reads its input one (stored) column to the right
        def shifted(xx, dd, kind, up):
            w, b = wl.wgrad_reference(xx, dd, kind, up)
            w2, _ = wl.wgrad_reference(F.pad(xx[..., 1:], (0, 1)), dd, kind, up)
            w = w.clone()
            w[:, :, 1, 1] = w2[:, :, 1, 1]
            return w, b
        w, b = (t.float() for t in wl.layer_reference(x, dy, case.kind, case.up, three, wgrad=shifted)[:2])
        moved = w != ref_w
        other = torch.ones(k, k, dtype=torch.bool)
        other[1, 1] = False
        assert not bool(moved[:, :, other].any()) and torch.equal(b, ref_b)
        assert bool(moved[:, :, 1, 1].any()), "a misplaced tap is a different number"
        # (by chance a shifted sum can equal the true one for single elements: most move, all of them need not)
        assert float(moved[:, :, 1, 1].float().mean()) > 0.5
