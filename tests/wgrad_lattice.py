"""Inputs for which a weight gradient is an EXACT sum, their float64 reference, and a runner for engine.WgradBatch (no test functions:
tests/test_wgrad_lattice_host.py checks this module on the CPU, tests/test_gpu_wgrad_exact.py holds the kernels to it).

A weight gradient is dW[co][ci][ky][kx] = alpha * sum over pixels of dY * X (include/ssr_hip.h).  With operands on a dyadic lattice every
product is a multiple of one granule 2^-g, and as long as sum |terms| < 2^24 granules every partial sum of every summation order is an
fp32 number: MFMA accumulation, the cross-wave reduce, fp32 atomics in arrival order and the fixed-order reduce of the deterministic mode
must then all give the bits of the float64 sum.  A missing, doubled or misplaced term is a different number, never a rounding.

  coarse  v = a + b / 16,   a in +-{1, 2, 3}, b in {-1, 0, 1}: 6 significant bits (exact in bf16), products are multiples of 2^-8
  split   v = a + b * 2^-9, same a, b: ssr_split_bf16 gives hi = a, lo = b * 2^-9 exactly.  Both fp32x3 forms compute
          dyh.xh + dyh.xl + dyl.xh (the lo.lo term is dropped by the mode's definition): multiples of 2^-9; db = sum dyh + sum dyl

The exactness condition is asserted for every case by `expected` (never skipped): margin = sum |terms| / granule / 2^24 < 1, the granule
including the power of two of alpha."""
import contextlib
import os
import zlib
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

KINDS = {"k3": (3, 1, 1), "k3p0": (3, 1, 0), "k4": (4, 2, 1)}      # (kernel size, stride, pad)
GRANULE_BITS = {"coarse": 8, "split": 9}


def rup(a, b):
    return (a + b - 1) // b * b


# ================================================================================================ lattices
def _lattice(shape, seed, step):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randint(1, 4, shape, generator=gen).double() * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)
    b = torch.randint(-1, 2, shape, generator=gen).double()
    return (a + b * step).float()


def coarse_lattice(shape, seed):
    return _lattice(shape, seed, 2.0 ** -4)


def split_lattice(shape, seed):
    return _lattice(shape, seed, 2.0 ** -9)


LATTICES = {"coarse": coarse_lattice, "split": split_lattice}


def split_planes(x):
    """hi = bf16(x), lo = bf16(x - hi), round to nearest even: the rule of ssr_split_bf16 (tests/test_gpu_support_helpers.py::_split_reference)"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.float(), lo.float()


# ================================================================================================ cases
@dataclass(frozen=True)
class Layer:
    cin: int                              # Cin_w: the channels of the weight
    cout: int
    alpha: float = 1.0
    x: Tuple[str, int] = ("x", 0)         # (input buffer, first channel of the view)
    dy: Optional[Tuple[str, int]] = None  # (gradient buffer, first channel); None: a buffer of its own of rup(cout, 8) channels
    cin_view: Optional[int] = None        # Cin: the channels of the view (a multiple of 8 >= cin); default rup(cin, 8)

    @property
    def cin_pad(self):
        return self.cin_view or rup(self.cin, 8)


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                             # key of KINDS
    B: int
    Hi: int                               # STORED input size (before the nearest x2 of up = 2)
    Wi: int
    layers: Tuple[Layer, ...]
    up: int = 1
    channels: Tuple[Tuple[str, int], ...] = ()      # channel counts of named buffers wider than their views need

    @property
    def grid(self):
        k, s, pad = KINDS[self.kind]
        return (self.Hi * self.up + 2 * pad - k) // s + 1, (self.Wi * self.up + 2 * pad - k) // s + 1

    @property
    def pixels(self):
        return self.B * self.grid[0] * self.grid[1]

    def buffers(self):
        """name -> (is_input, channels, [(first, data channels, view channels)])"""
        out, given = {}, dict(self.channels)
        for i, L in enumerate(self.layers):
            for is_x, (name, coff), nc, ncp in ((True, L.x, L.cin, L.cin_pad), (False, L.dy or (f"dy{i}", 0), L.cout, rup(L.cout, 8))):
                b = out.setdefault(name, [is_x, given.get(name, 0), []])
                assert b[0] == is_x, "a buffer is an input or a gradient, not both"
                b[1] = max(b[1], coff + ncp)
                b[2].append((coff, nc, ncp))
        return out


def _case(name, kind, B, hw, layers, **kw):
    layers = tuple(Layer(*L) if isinstance(L, tuple) else L for L in layers)
    return Case(name, kind, B, hw[0], hw[1], layers, **kw)


def k3_case(name, B, grid, layers, pad=1, up=1, **kw):
    """3x3 stride 1 by its output grid: pad 1 reads a grid-sized input, pad 0 (the L2 models' form) an (H + 2) x (W + 2) one"""
    assert grid[0] % up == 0 and grid[1] % up == 0
    hw = (grid[0] // up, grid[1] // up) if pad else (grid[0] + 2, grid[1] + 2)
    return _case(name, "k3" if pad else "k3p0", B, hw, layers, up=up, **kw)


def k4_case(name, B, hw_in, layers, **kw):
    return _case(name, "k4", B, hw_in, layers, **kw)


def dense_layers(alphas=(1.0, 1.0, 0.5, 1.0, 0.25)):
    """a dense block's five convs (the DENSE of tests/test_gpu_wgrad_x3.py) as the engine lays them out: conv1..4 read the leading 64..160
    channels of the 192-channel buffer "x" and their output gradients sit at channels 64..160 of the 192-channel buffer "g" (whose first
    64 channels no layer reads); conv5 reads all 192 and has a gradient buffer of its own"""
    ls = [Layer(64 + 32 * k, 32, alphas[k], ("x", 0), ("g", 64 + 32 * k)) for k in range(4)]
    return tuple(ls + [Layer(192, 64, alphas[4], ("x", 0), None)])


DENSE_CHANNELS = (("x", 192), ("g", 192))

# ---- the shared case lists (tests/test_gpu_wgrad_exact.py runs them, tests/test_wgrad_lattice_host.py checks the condition for each) ----
ONE = ((64, 32),)
GRID_K3 = [k3_case(f"grid-k3-{B}x{h}x{w}", B, (h, w), ONE) for B in (1, 2) for h, w in ((16, 16), (17, 15), (15, 17), (1, 1), (2, 3), (33, 16))]
GRID_K3P0 = [k3_case(f"grid-k3p0-{B}x{h}x{w}", B, (h, w), ONE, pad=0) for B in (1, 2)
             for h, w in ((16, 16), (17, 15), (15, 17), (1, 1), (2, 3), (33, 16))]
GRID_K4 = [k4_case(f"grid-k4-{B}x{h}x{w}", B, (h, w), ONE) for B in (1, 2) for h, w in ((32, 32), (34, 30), (2, 2), (6, 66), (5, 8))]

# Tiles per item against the ring of NST stages: 1, NST, NST + 1 and 2 NST + 1 tiles per item over B = 3 images whose tile count (in the
# tile size of the kernel) no such range divides into, so that ranges begin and end in the middle of an image; ragged in both directions;
# 64 -> 64 so that the kernels that pair have pairs.  WgradBatch.add cuts `tiles` into ceil(tiles / cap) EVEN ranges, so the totals are
# chosen such that the even range IS the cap: 18 tiles for caps 1, 2, 3, 5 (NST = 2), 27 tiles for caps 1, 3, 4, 7 (NST = 3).
# key (mode, kind) -> (case, tile rows, tile grid of one image)
_T16 = k3_case("tiles-k3-th16", 3, (35, 20), ((64, 64),))        # 16 x 16 tiles: 3 x 2 per image
_T8 = k3_case("tiles-k3-th8", 3, (19, 20), ((64, 64),))          # 8 x 16 tiles: 3 x 2
_T48 = k4_case("tiles-k4-th8", 3, (38, 40), ((64, 64),))         # 4x4 stride 2, 19 x 20 outputs in 8 x 16 tiles: 3 x 2
_T489 = k4_case("tiles-k4-th8-9", 3, (38, 72), ((64, 64),))      # 19 x 36 outputs in 8 x 16 tiles: 3 x 3
_T44 = k4_case("tiles-k4-th4", 3, (22, 40), ((64, 64),))         # 11 x 20 outputs in 4 x 16 tiles: 3 x 2
TILE_CASES = {
    ("bf16", "k3"): (_T16, 16, (3, 2)), ("x3pass", "k3"): (_T16, 16, (3, 2)), ("fp32", "k3"): (_T8, 8, (3, 2)), ("x3", "k3"): (_T8, 8, (3, 2)),
    ("bf16", "k4"): (_T489, 8, (3, 3)), ("x3pass", "k4"): (_T489, 8, (3, 3)), ("fp32", "k4"): (_T48, 8, (3, 2)), ("x3", "k4"): (_T44, 4, (3, 2)),
}


def ring_stages(mode, kind):
    """NST of the kernel a mode runs, as read from the code: Wg3::NST = 2 (csrc/wgrad_bf16.hip, 3x3), Wx3::NST = Wx4::NST = 2
    (csrc/wgrad_x3.hip), and WgCfg<4, 4, 2, true>::NST = min(4, 156 KB / STAGE) with STAGE = 16 B x (4 vectors per pixel) x (8 x 16 dY
    pixels + 18 x 34 patch pixels) = 47,360 B: 3.  The exact-fp32 kernel (csrc/wgrad.hip) has no ring: it gets the counts of NST = 2."""
    if mode in ("bf16", "x3pass") and kind == "k4":
        th, ph, pw = 8, 7 * 2 + 4, 15 * 2 + 4
        return min(4, 156 * 1024 // (16 * 4 * (th * 16 + ph * pw)))
    return 2

_CH = ((3, 64), (64, 3), (64, 1), (24, 40), (96, 32), (40, 72))
# Cin_w < Cin throughout: the view is the next multiple of 8 past cin + 1
CHANNEL_K3 = [k3_case(f"ch-k3-{ci}-{co}", 2, (9, 7), (Layer(ci, co, cin_view=rup(ci + 1, 8)),)) for ci, co in _CH] + \
             [k3_case("ch-k3-512-256", 1, (4, 4), (Layer(512, 256, cin_view=520),))]
CHANNEL_K4 = [k4_case(f"ch-k4-{ci}-{co}", 2, (10, 14), (Layer(ci, co, cin_view=rup(ci + 1, 8)),)) for ci, co in _CH] + \
             [k4_case("ch-k4-512-256", 1, (8, 8), (Layer(512, 256, cin_view=520),))]

DENSE_CASES = [k3_case(f"dense-2x{h}x{w}", 2, (h, w), dense_layers(), channels=DENSE_CHANNELS) for h, w in ((13, 21), (32, 32))]
# SSR_WGRAD_BALANCE recuts a paired item only past 32 tiles (wgrad_plan.balance): nine images of 2 x 2 ragged 16 x 16 tiles
DENSE_BALANCE = k3_case("dense-9x17x17", 9, (17, 17), dense_layers(), channels=DENSE_CHANNELS)
# the first dense conv alone: its 64-channel views lie inside the 192-channel buffers, every other channel is NaN
DENSE_FIRST = k3_case("dense-first-2x13x21", 2, (13, 21), dense_layers()[:1], channels=DENSE_CHANNELS)

UP2_CASES = [k3_case(f"up2-2x{h}x{w}", 2, (2 * h, 2 * w), ((64, 64),), up=2) for h, w in ((9, 7), (16, 16))]

ACCUM_K3 = k3_case("accum-k3", 2, (17, 15), ((64, 64), (24, 40)))
ACCUM_K4 = k4_case("accum-k4", 2, (34, 30), ((64, 64),))
RANDOM_CASE = k3_case("random-3x13x21", 3, (13, 21), ((64, 64, 0.5), (40, 24)))

# (case, lattice, launches, prefilled): everything the GPU file runs
ALL_CASES = []
for _c in GRID_K3 + GRID_K3P0 + GRID_K4 + CHANNEL_K3 + CHANNEL_K4 + DENSE_CASES + [DENSE_BALANCE, DENSE_FIRST] + UP2_CASES + \
        [_T16, _T8, _T48, _T489, _T44]:
    ALL_CASES += [(_c, "coarse", 1, False), (_c, "split", 1, False)]
for _c in (ACCUM_K3, ACCUM_K4):
    for _lat in ("coarse", "split"):
        ALL_CASES += [(_c, _lat, 1, False), (_c, _lat, 2, False), (_c, _lat, 1, True)]


# ================================================================================================ inputs
def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def fill_buffer(values, views):
    """values [..., C] -> the buffer the kernels see: the data channels of every view keep their values, the padding channels inside a
    view (Cin_w..Cin, Cout..rup(Cout, 8)) are zero, every channel no view covers is NaN (an over-read poisons the result)"""
    C = values.shape[-1]
    data, pad = torch.zeros(C, dtype=torch.bool), torch.zeros(C, dtype=torch.bool)
    for coff, nc, ncp in views:
        data[coff:coff + nc] = True
        pad[coff + nc:coff + ncp] = True
    assert not bool((data & pad).any()), "one view's padding channels are another's data"
    out = values.clone()
    out[..., pad] = 0.0
    out[..., ~(data | pad)] = float("nan")
    return out


@lru_cache(maxsize=None)
def inputs(case, lattice):
    """name -> fp32 NHWC CPU tensor (shared between tests: do not modify); `lattice` may also be "randn" (the one random-data test)"""
    gh, gw = case.grid
    out = {}
    for name, (is_x, C, views) in case.buffers().items():
        shape = (case.B, case.Hi, case.Wi, C) if is_x else (case.B, gh, gw, C)
        if lattice == "randn":
            v = torch.randn(shape, generator=torch.Generator().manual_seed(_seed(case.name, name))) * (0.5 if is_x else 0.25)
        else:
            v = LATTICES[lattice](shape, _seed(case.name, name, lattice))
        out[name] = fill_buffer(v, views)
    return out


@lru_cache(maxsize=None)
def prefill(case):
    """small integers already in the gradients (D's fake pass adds to what its real pass left): [(dW, db)] fp32"""
    k = KINDS[case.kind][0]
    out = []
    for i, L in enumerate(case.layers):
        gen = torch.Generator().manual_seed(_seed(case.name, "prefill", i))
        out.append((torch.randint(-8, 9, (L.cout, L.cin, k, k), generator=gen).float(), torch.randint(-8, 9, (L.cout,), generator=gen).float()))
    return out


# ================================================================================================ float64 reference
def wgrad_reference(x, dy, kind, up=1):
    """x [B, Cin, Hi, Wi], dy [B, Cout, Gh, Gw] float64 -> (dW [Cout, Cin, k, k], db [Cout]): autograd of F.conv2d (F.interpolate in front
    for up = 2), alpha not applied"""
    k, s, pad = KINDS[kind]
    if up == 2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w = torch.zeros(dy.shape[1], x.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(dy.shape[1], dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, b, stride=s, padding=pad)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    (y * dy).sum().backward()
    return w.grad, b.grad


def layer_operands(case, data, i):
    """(x [B, cin, Hi, Wi], dy [B, cout, Gh, Gw]) float64 of layer i: the data channels of its two views"""
    L = case.layers[i]
    (xn, xo), (gn, go) = L.x, L.dy or (f"dy{i}", 0)
    x = data[xn][..., xo:xo + L.cin].double().permute(0, 3, 1, 2)
    dy = data[gn][..., go:go + L.cout].double().permute(0, 3, 1, 2)
    return x, dy


def term_pairs(x, dy, three_term):
    """the (x, dy) operand pairs whose gradients add up to the mode's result: one, or the three of the fp32x3 forms"""
    if not three_term:
        return [(x, dy)]
    (xh, xl), (dh, dl) = split_planes(x.float()), split_planes(dy.float())
    return [(xh.double(), dh.double()), (xl.double(), dh.double()), (xh.double(), dl.double())]


def layer_reference(x, dy, kind, up, three_term, wgrad=wgrad_reference):
    """-> (dW, db, sum |terms| of dW, sum |terms| of db) in float64, alpha not applied"""
    dw = db = aw = ab = 0.0
    for n, (xx, dd) in enumerate(term_pairs(x, dy, three_term)):
        w, b = wgrad(xx, dd, kind, up)
        a, c = wgrad(xx.abs(), dd.abs(), kind, up)
        dw, aw = dw + w, aw + a
        if n != 1:                                         # db = sum dy_hi + sum dy_lo: the pairs 0 and 2
            db, ab = db + b, ab + c
    return dw, db, aw, ab


@lru_cache(maxsize=None)
def reference(case, lattice, three_term):
    data = inputs(case, lattice)
    return [layer_reference(*layer_operands(case, data, i), case.kind, case.up, three_term) for i in range(len(case.layers))]


def _alpha_bits(alpha):
    """alpha = m * 2^-e with a small integer m -> e (scaling by it is exact and refines the granule by e bits)"""
    fr = Fraction(alpha)
    e = fr.denominator.bit_length() - 1
    assert fr.denominator == 1 << e and abs(fr.numerator) <= 8, f"alpha {alpha} is no small multiple of a power of two"
    return e


def expected(case, lattice, three_term, launches=1, prefilled=False, with_bias=True):
    """-> ([(dW, db)] fp32, margin).  Asserts the exactness condition, sum |terms| * 2^g < 2^24 for every output element (prefilled
    values and repeated launches included), and that the float64 result is an fp32 number."""
    g = GRANULE_BITS[lattice]
    out, margin = [], 0.0
    for L, (dw, db, aw, ab), (pw, pb) in zip(case.layers, reference(case, lattice, three_term), prefill(case)):
        scale = 2.0 ** (g + _alpha_bits(L.alpha)) / 2.0 ** 24
        res = []
        for val, mag, pre, on in ((dw, aw, pw, True), (db, ab, pb, with_bias)):
            pre = pre.double() if prefilled else torch.zeros_like(val)
            e = pre + (launches * L.alpha * val if on else 0.0)
            m = float((pre.abs() + launches * abs(L.alpha) * mag).max()) * scale
            assert m < 1.0, f"{case.name}/{lattice}: sum |terms| is {m:.3f} of 2^24 granules: the sum is not exact in every order"
            assert torch.equal(e.float().double(), e), f"{case.name}/{lattice}: the expected value is no fp32 number"
            margin = max(margin, m)
            res.append(e.float())
        out.append(tuple(res))
    return out, margin


# ================================================================================================ the runner
# mode -> (dtype name of hip, lattice, three-term expectation, environment of the batch)
MODES = {
    "bf16": ("BF16", "coarse", False, {}),
    "fp32": ("F32", "coarse", False, {}),
    "x3pass": ("F32X3", "split", True, {"SSR_X3_WGRAD_FUSED": "0", "SSR_X3_WGRAD_FUSED4": "0"}),      # the bf16 kernel three times over hi / lo planes
    "x3": ("F32X3", "split", True, {"SSR_X3_WGRAD_FUSED": "1", "SSR_X3_WGRAD_FUSED4": "1"}),          # csrc/wgrad_x3.hip
}


@contextlib.contextmanager
def environ(values):
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tile_rows(mode, kind):
    """rows of the 16-pixel-wide tile of the kernel a mode runs (csrc/wgrad_common.h, wgrad_bf16.hip, wgrad_x3.hip)"""
    k = KINDS[kind][0]
    if mode in ("bf16", "x3pass"):
        return 16 if k == 3 else 8
    return 4 if (mode == "x3" and k == 4) else 8


def run(case, mode, *, data=None, det=False, force_atomic=False, tiles_per_item=None, with_bias=True, prefilled=False, launches=1,
        env=None, odd_parent=False):
    """One engine.WgradBatch over the layers of `case` (the shape of _run / _run4 of tests/test_gpu_wgrad_x3.py), launched `launches` times.
    dW / db lie between sentinel margins (Guarded of tests/test_gpu_support_kernels.py); `tiles_per_item` becomes MAX_TILES_PER_ITEM of
    the instance in units of the kernel's own tiles; `odd_parent`: every buffer is the leading part of an allocation of numel() % 8 == 4.
    -> wb, grads [(dW, db)] fp32 CPU, guards_ok, inputs_ok, tiles (per layer, in the kernel's tiles)"""
    from satlas_super_resolution_amd import engine, hip
    from test_gpu_support_kernels import guarded_from, same_bits
    dtname, lattice, _, menv = MODES[mode]
    dtype = getattr(hip, dtname)
    tdt = torch.bfloat16 if dtype == hip.BF16 else torch.float32
    k, s, pad = KINDS[case.kind]
    gh, gw = case.grid
    data = inputs(case, lattice) if data is None else data
    keep, dev = [], {}
    for name, t in data.items():
        flat = torch.full((t.numel() + (4 if odd_parent else 0),), float("nan"), dtype=tdt, device="cuda")
        if odd_parent:
            hip.view(flat)                                 # the whole allocation is the parent the split passes find
        dev[name] = flat[:t.numel()].view(t.shape)
        dev[name].copy_(t)
        keep.append(flat)
    before = {name: t.clone() for name, t in dev.items()}
    grads = []
    with environ({**menv, **(env or {})}):
        wb = engine.WgradBatch(dtype, k, s, force_atomic=force_atomic, det=det)
        assert wb.kdt == {"x3pass": hip.BF16, "x3": hip.F32X3}.get(mode, dtype), "the kernel the mode is named after"
        if tiles_per_item:
            # add() doubles the cap for the one-pass kernels (their tiles are half the bf16 kernels'): halve it here
            wb.MAX_TILES_PER_ITEM = {k: Fraction(tiles_per_item, 2 if wb.kdt == hip.F32X3 else 1)}
        for i, L in enumerate(case.layers):
            (xn, xo), (gn, go) = L.x, L.dy or (f"dy{i}", 0)
            pw, pb = prefill(case)[i]
            dw = guarded_from(pw if prefilled else torch.zeros_like(pw))
            db = guarded_from(pb if prefilled else torch.zeros_like(pb))
            wb.add(hip.view(dev[xn], xo), hip.view(dev[gn], go), case.B, case.Hi, case.Wi, case.up, L.cin_pad, L.cout, gh, gw, L.alpha,
                   dw.ptr(), L.cin, db.ptr() if with_bias else None, pad=pad)
            grads.append((dw, db))
        wb.finalize()
    launcher = engine.Launcher()
    wb.launch(launcher)
    for _ in range(launches):
        launcher.run()
    torch.cuda.synchronize()
    return SimpleNamespace(
        wb=wb, keep=keep,
        grads=[(dw.t.cpu().view(L.cout, L.cin, k, k), db.t.cpu()) for (dw, db), L in zip(grads, case.layers)],
        guards_ok=all(dw.margins_intact() and db.margins_intact() for dw, db in grads),
        inputs_ok=all(same_bits(dev[name], before[name]) for name in dev),
        tiles=hip.lib().ssr_wgrad_tiles(case.B, gh, gw, wb.kdt, k))


def margin_line(case, lattice, three_term, launches, prefilled):
    _, m = expected(case, lattice, three_term, launches, prefilled)
    tag = f"{case.name} {lattice}{' x' + str(launches) if launches > 1 else ''}{' prefilled' if prefilled else ''}"
    return f"{tag}: {case.pixels} pixels, sum |terms| = {m:.4f} of 2^24 granules"
