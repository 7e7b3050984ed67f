"""GPU: the bf16 (csrc/wgrad_bf16.hip), exact-fp32 (csrc/wgrad.hip), three-pass fp32x3 (engine.WgradBatch over hi / lo planes) and
one-pass fp32x3 (csrc/wgrad_x3.hip) weight gradients held to EXACT sums.  The inputs lie on the dyadic lattices of
tests/wgrad_lattice.py, for which every product and every partial sum of every summation order is an fp32 number: MFMA accumulation,
cross-wave reduce, fp32 atomics in arrival order and the fixed-order reduce must all give the bits of the float64 reference.

Every case asserts (1) torch.equal on dW and db, no tolerance; (2) the sentinel margins around dW / db and the input buffers unchanged;
(3) the property of the item table it is about, so that it cannot silently stop exercising its path.  Channels of the parent buffers
that no view covers are NaN: an over-read poisons the result.  The exactness condition of every case is asserted by
wgrad_lattice.expected (and for the whole list, on the CPU, by tests/test_wgrad_lattice_host.py).

One test uses random data (the three-pass form against float64 at the 1e-4 of tests/test_gpu_wgrad_x3.py): lattice data cannot see a
wrong rounding inside the split itself."""
import pytest
import torch

import wgrad_lattice as wl
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4                                     # tests/test_gpu_wgrad_x3.py
PAIRING = ("bf16", "x3pass", "x3")             # modes whose 3x3 kernel takes paired items (ssr_wgrad_co_tile == 64)


def _name(c):
    return c.name


def check(case, mode, res, **kw):
    """bit-exact against the float64 sum, guards and inputs intact"""
    _, lattice, three, _ = wl.MODES[mode]
    exp, margin = wl.expected(case, lattice, three, **kw)
    g = wl.GRANULE_BITS[lattice]
    for i, ((dw, db), (ew, eb)) in enumerate(zip(res.grads, exp)):
        for what, got, want in (("dW", dw, ew), ("db", db, eb)):
            if not torch.equal(got, want):
                bad = (got != want) | torch.isnan(got)
                first = tuple(int(v) for v in bad.nonzero()[0])
                raise AssertionError(f"{case.name} {mode} layer {i} {what}: {int(bad.sum())} of {bad.numel()} elements differ, first at "
                                     f"{first}: got {float(got[first])!r}, want {float(want[first])!r}; largest difference "
                                     f"{float(torch.nan_to_num((got - want).abs(), nan=float('inf')).max()) * 2 ** g:g} granules (margin {margin:.3f})")
    assert res.guards_ok, "a write outside dW / db"
    assert res.inputs_ok, "an input buffer was written"


def n_items(res, case, paired=False):
    """items of single-split layers: one per (32 co, ci tile); `paired`: the blocks of ONE layer two by two, an odd one left single"""
    from satlas_super_resolution_amd import hip
    wb = res.wb
    ci_tile = hip.lib().ssr_wgrad_ci_tile(wb.kdt, wb.k)
    blocks = lambda L: -(-L.cout // 32)      # noqa: E731
    return sum(((blocks(L) + 1) // 2 if paired else blocks(L)) * -(-L.cin // ci_tile) for L in case.layers)


# ================================================================================================ grid edges
@pytest.mark.parametrize("case", wl.GRID_K3 + wl.GRID_K4, ids=_name)
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass"])
def test_grid_edges(mode, case):
    """one layer 64 -> 32 on grids of exactly one tile, one row / column more or less, a single pixel, 2 x 3, three tile rows; 4x4 stride 2
    on even, ragged, minimal, wide and odd-height inputs.  One item per (co, ci) tile walks all images: no atomics, no partials."""
    res = wl.run(case, mode)
    gh, gw = case.grid
    assert res.tiles == case.B * -(-gh // wl.tile_rows(mode, case.kind)) * -(-gw // 16), "the tile size this file assumes is the kernel's"
    assert len(res.wb.items) == n_items(res, case) and all(it.atomic == 0 and it.nco <= 1 for it in res.wb.items)
    assert all((it.tile_begin, it.tile_end) == (0, res.tiles) for it in res.wb.items) and res.wb.partial is None
    check(case, mode, res)


@pytest.mark.parametrize("case", wl.GRID_K3P0, ids=_name)
def test_grid_edges_pad0_fp32_deterministic(case):
    """the form of archs/l2_archs.py: pad 0 over an (H + 2) x (W + 2) input, exact fp32, deterministic mode (partials from five tiles on)"""
    res = wl.run(case, "fp32", det=True, tiles_per_item=4)
    L = res.wb.layers[0]
    assert (L.pad_y, L.pad_x) == (0, 0) and (L.Hi, L.Wi) == (L.Gh + 2, L.Gw + 2) and res.wb.det
    assert (res.wb.partial is not None) == (res.tiles > 4) and all(it.atomic == 0 for it in res.wb.items)
    check(case, "fp32", res)


# ================================================================================================ tiles per item against the ring
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("which", ["1", "nst", "nst+1", "2nst+1"])
@pytest.mark.parametrize("kind", ["k3", "k4"])
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass", "x3"])
def test_tiles_per_item_against_the_ring(mode, kind, which, det):
    """1, NST, NST + 1 and 2 NST + 1 tiles per item: the ring is not filled, filled once, wraps by one stage, wraps twice and ends on its
    first stage.  The ranges begin and end in the middle of an image (its halo rows must not come from the neighbouring image), the
    splits of a layer meet in dW through atomics or through the partial buffers of the deterministic mode."""
    case, th, (ty, tx) = wl.TILE_CASES[(mode, kind)]
    nst = wl.ring_stages(mode, kind)
    t = {"1": 1, "nst": nst, "nst+1": nst + 1, "2nst+1": 2 * nst + 1}[which]
    res = wl.run(case, mode, det=det, tiles_per_item=t)
    items = res.wb.items
    assert res.tiles == case.B * ty * tx
    assert max(it.tile_end - it.tile_begin for it in items) == t and sum(it.tile_end - it.tile_begin == t for it in items) > len(items) // 2
    assert any(it.tile_begin % (ty * tx) for it in items) and any(it.tile_end % (ty * tx) for it in items), "ranges cut inside an image"
    if det:
        assert res.wb.partial is not None and max(it.atomic for it in items) == 0 and len(res.wb.virtual) == -(-res.tiles // t)
    else:
        assert res.wb.partial is None and min(it.atomic for it in items) == 1
    if mode in PAIRING and (kind == "k3" or mode == "x3"):
        assert all(it.nco == 2 and it.layer == it.layer_b for it in items), "the halves of the 64-output conv share an item"
    check(case, mode, res)


# ================================================================================================ channel edges
@pytest.mark.parametrize("case", wl.CHANNEL_K3 + wl.CHANNEL_K4, ids=_name)
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass"])
def test_channel_edges(mode, case):
    """thin inputs and outputs, half-filled channel tiles (96: the second 64-wide input tile is half full), three output blocks (72: a pair
    and a single where the kernel pairs), many (co, ci) tiles on a 4 x 4 grid; the view is wider than the weight throughout"""
    res = wl.run(case, mode)
    L, spec = res.wb.layers[0], case.layers[0]
    assert L.Cin_w < L.Cin and L.Cin % 8 == 0 and (L.Cin_w, L.Cout) == (spec.cin, spec.cout)
    paired = mode in PAIRING and case.kind == "k3"
    assert len(res.wb.items) == n_items(res, case, paired) and all(it.atomic == 0 for it in res.wb.items)
    if spec.cout == 72 and paired:
        assert any(it.nco == 2 for it in res.wb.items) and any(it.nco <= 1 for it in res.wb.items)
    if spec.cin == 512:
        assert len(res.wb.items) >= 8 * 8 // 2
    check(case, mode, res)


# ================================================================================================ dense block
def _dense_properties(mode, res):
    wb = res.wb
    assert all(L.x.cs == 192 and L.x.coff == 0 for L in wb.layers) and sorted(L.dy.coff for L in wb.layers) == [0, 64, 96, 128, 160]
    assert sorted(L.alpha for L in wb.layers) == [0.25, 0.5, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("case", wl.DENSE_CASES, ids=_name)
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass", "x3"])
def test_dense_block(mode, case):
    """the five convs of a dense block over one 192-channel buffer, output gradients as views at channels 64..160 of another (its first 64
    channels are NaN), alpha 1, 0.5 and 0.25"""
    res = wl.run(case, mode)
    _dense_properties(mode, res)
    if mode in PAIRING:
        assert any(it.nco == 2 and it.layer != it.layer_b for it in res.wb.items), "two layers share an item"
        assert any(it.nco == 2 and it.layer == it.layer_b for it in res.wb.items), "the halves of the 64-output conv share an item"
    else:
        assert all(it.nco <= 1 for it in res.wb.items)
    check(case, mode, res)


def _item_key(it):
    return (it.layer, it.co0, it.ci0, it.tile_begin, it.tile_end, it.atomic, it.nco, it.layer_b, it.co0_b)


@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass", "x3"])
def test_dense_block_bits_do_not_depend_on_pairing_or_launch_order(mode):
    """SSR_WGRAD_PAIR=0, SSR_WGRAD_BALANCE=1 and every SSR_WGRAD_ORDER: other items, another order, the same bits"""
    from satlas_super_resolution_amd import wgrad_plan
    case = wl.DENSE_CASES[0]
    res = wl.run(case, mode, env={"SSR_WGRAD_PAIR": "0"})
    assert all(it.nco <= 1 for it in res.wb.items) and len(res.wb.items) == n_items(res, case)
    check(case, mode, res)
    # SSR_WGRAD_BALANCE=1 at this size: the simulation runs and keeps the items whole (test_dense_block_balanced_items is where it recuts)
    res = wl.run(case, mode, env={"SSR_WGRAD_BALANCE": "1"})
    assert hasattr(res.wb, "balance_choice") == (mode in PAIRING) and all(it.tile_end - it.tile_begin == res.tiles for it in res.wb.items)
    check(case, mode, res)
    orders = {}
    for key in wgrad_plan.ORDERS:
        res = wl.run(case, mode, env={"SSR_WGRAD_ORDER": key})
        _dense_properties(mode, res)
        orders[key] = [_item_key(it) for it in res.wb.items]
        check(case, mode, res)
    assert len({tuple(sorted(o)) for o in orders.values()}) == 1, "the same items"
    assert len({tuple(o) for o in orders.values()}) > 1, "in more than one order"


@pytest.mark.parametrize("mode", PAIRING)
def test_dense_block_balanced_items(mode):
    """SSR_WGRAD_BALANCE=1 recuts the items into finer pixel ranges that meet through atomics (wgrad_plan.balance; past 32 tiles a pair)"""
    case = wl.DENSE_BALANCE
    plain = wl.run(case, mode)
    res = wl.run(case, mode, env={"SSR_WGRAD_BALANCE": "1"})
    assert res.wb.balance_choice[2] < res.wb.balance_choice[3], "the simulation chose a finer cut"
    assert len(res.wb.items) > len(plain.wb.items) and max(it.atomic for it in plain.wb.items) == 0
    assert any(it.nco == 2 and it.atomic == 1 and it.tile_end - it.tile_begin < res.tiles for it in res.wb.items)
    check(case, mode, plain)
    check(case, mode, res)


@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass", "x3"])
def test_views_inside_buffers_of_nan(mode):
    """the first dense conv alone: 64-channel views (dY at channel 64) of 192-channel buffers whose other channels are NaN"""
    case = wl.DENSE_FIRST
    res = wl.run(case, mode)
    L = res.wb.layers[0]
    assert (L.x.cs, L.x.coff, L.Cin, L.dy.cs, L.dy.coff, L.Cout) == (192, 0, 64, 192, 64, 32)
    assert all(bool(torch.isnan(t).any()) for t in res.keep)
    check(case, mode, res)


# ================================================================================================ up = 2
@pytest.mark.parametrize("case", wl.UP2_CASES, ids=_name)
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass"])
def test_nearest_upsampling_folded_into_the_read(mode, case):
    res = wl.run(case, mode)
    L = res.wb.layers[0]
    assert L.up == 2 and (L.Gh, L.Gw) == (2 * L.Hi, 2 * L.Wi)
    check(case, mode, res)


# ================================================================================================ accumulation
@pytest.mark.parametrize("case", [wl.ACCUM_K3, wl.ACCUM_K4], ids=_name)
@pytest.mark.parametrize("mode", ["bf16", "fp32", "x3pass", "x3"])
class TestAccumulation:
    def test_two_launches_give_exactly_twice(self, mode, case):
        res = wl.run(case, mode, launches=2)
        check(case, mode, res, launches=2)

    def test_two_launches_of_the_deterministic_mode(self, mode, case):
        res = wl.run(case, mode, launches=2, det=True, tiles_per_item=2)
        assert res.wb.partial is not None
        check(case, mode, res, launches=2)

    def test_into_prefilled_gradients(self, mode, case):
        """what D's fake pass does to the gradients of its real pass"""
        res = wl.run(case, mode, prefilled=True)
        check(case, mode, res, prefilled=True)

    def test_without_bias_db_stays_untouched(self, mode, case):
        res = wl.run(case, mode, prefilled=True, with_bias=False)
        assert all(L.db is None for L in res.wb.layers)
        for (_, db), (_, pb) in zip(res.grads, wl.prefill(case)):
            assert torch.equal(db, pb)
        check(case, mode, res, prefilled=True, with_bias=False)

    def test_force_atomic(self, mode, case):
        res = wl.run(case, mode, force_atomic=True, prefilled=True)
        assert min(it.atomic for it in res.wb.items) == 1 and res.wb.partial is None
        check(case, mode, res, prefilled=True)


# ================================================================================================ the fp32x3 forms
def test_three_pass_splits_each_buffer_when_one_is_no_multiple_of_eight():
    """a parent buffer of numel() % 8 == 4: _launch_wgrad issues ssr_split_bf16 per buffer instead of ssr_split_bf16_multi"""
    case = next(c for c in wl.GRID_K3 if c.name == "grid-k3-2x17x15")
    res = wl.run(case, "x3pass", odd_parent=True)
    wb = res.wb
    assert len(wb.splits) == 2 and all(p.numel() % 8 == 4 for p, _, _ in wb.splits) and wb.split_tab is None
    assert wb.kdt != wb.dtype and len(wb.split_tabs) == 3
    check(case, "x3pass", res)
    res = wl.run(case, "x3pass")
    assert res.wb.split_tab is not None and all(p.numel() % 8 == 0 for p, _, _ in res.wb.splits)
    check(case, "x3pass", res)


@pytest.mark.parametrize("kind", ["k3", "k4"])
def test_one_pass_and_three_pass_forms_give_identical_bits(kind):
    """both compute dyh.xh + dyh.xl + dyl.xh; on the split lattice both are exact, so they are identical"""
    from satlas_super_resolution_amd import hip
    cases = [(wl.TILE_CASES[("x3", kind)][0], 3)] + ([(wl.DENSE_CASES[0], None)] if kind == "k3" else [])
    for case, t in cases:
        one = wl.run(case, "x3", tiles_per_item=t)
        three = wl.run(case, "x3pass", tiles_per_item=t)
        assert one.wb.kdt == hip.F32X3 and three.wb.kdt == hip.BF16 and one.wb.dtype == three.wb.dtype == hip.F32X3
        for (w1, b1), (w3, b3) in zip(one.grads, three.grads):
            assert torch.equal(w1, w3) and torch.equal(b1, b3)
        check(case, "x3", one)
        check(case, "x3pass", three)


def test_three_pass_form_on_random_data():
    """random data sees what the lattice cannot: a wrong rounding in the split.  Against float64 at the gate of tests/test_gpu_wgrad_x3.py
    (a product rounds at 2^-16); ragged grid, ranges of two tiles"""
    case = wl.RANDOM_CASE
    data = wl.inputs(case, "randn")
    res = wl.run(case, "x3pass", data=data, tiles_per_item=2)
    assert max(it.atomic for it in res.wb.items) == 1 and res.guards_ok and res.inputs_ok
    for i, ((dw, db), L) in enumerate(zip(res.grads, case.layers)):
        rw, rb = wl.wgrad_reference(*wl.layer_operands(case, data, i), case.kind, case.up)
        ew, eb = rel_err(dw.double(), L.alpha * rw), rel_err(db.double(), L.alpha * rb)
        print(f"\nthree-pass fp32x3, randn, layer {i}: dW {ew:.2e}, db {eb:.2e} of max|ref| (gate {TOL:g})", end="")
        assert ew < TOL and eb < TOL
