"""GPU: the helper kernels with bit-exact targets - ssr_wgrad_reduce (a fixed summation order), ssr_split_bf16 / _multi (two roundings to
nearest even), ssr_fill, ssr_add_views, ssr_axpby_f32 - and ssr_pack_weights against a host restatement of the packed layouts that
include/ssr_hip.h and csrc/misc.hip document.  Conventions (unit roundoff U, sentinel margins, sizes past the grid caps) as in
tests/test_gpu_support_kernels.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_support_kernels import (ADAM_CAP, ADAM_PER_BLOCK, EINVAL, EUNSUP, U, Guarded, _hip, _report_file, guarded_from,  # noqa: F401
                                      ibits, note, past_cap, read_view, same_bits, strided, within)

pytestmark = pytest.mark.gpu

# grid caps of csrc/misc.hip
REDUCE_PER_BLOCK, REDUCE_CAP = 256 * 4, 64            # ssr_wgrad_reduce: grid_for(max_elems, 256 * 4, 64)
SPLIT_PER_BLOCK, SPLIT_CAP = 256 * 4, 8192            # ssr_split_bf16: grid_for(n / 4, 256, 8192), 4 elements per thread
MULTI_PER_BLOCK, MULTI_CAP = 256 * 8, 2048            # ssr_split_bf16_multi: grid_for(max_n / 8, 256, 2048), 8 elements per thread
FILL_PER_BLOCK, FILL_CAP = 256, 4096                  # ssr_fill: grid_for(n) = grid_for(n, 256, 4096)
ADDV_PER_BLOCK, ADDV_CAP = 256 * 4, 2048              # ssr_add_views: grid_for(npix * C, 256 * 4, 2048)


# ================================================================================================ ssr_wgrad_reduce
def test_wgrad_reduce_is_the_fixed_order_sum():
    """dst[e] += src[0][e] + src[1][e] + ... in that order: additions only, so nothing can be fused and the numpy float32 loop is a
    bit-exact target.  Items of different n and parts in one table (max_elems exceeds most), stride > n, n past the 64-block cap."""
    hip, L = _hip()
    gen = torch.Generator().manual_seed(0)
    shapes = [(1, 1), (1, 7), (100003, 2), (past_cap(REDUCE_PER_BLOCK, REDUCE_CAP), 7), (4099, 7), (777, 1)]     # (n, parts)
    bufs, items = [], []
    for n, parts in shapes:
        stride = n + 13                                             # the gap between two parts holds values that must not be added
        dst0 = torch.randn(n, generator=gen)
        src = torch.randn(parts * stride, generator=gen) * 10 ** torch.randint(-3, 3, (parts * stride,), generator=gen).float()
        gd, gs = guarded_from(dst0), guarded_from(src)
        items.append(hip.ReduceItem(gd.ptr(), gs.ptr(), n, stride, parts, 0))
        bufs.append((gd, gs, dst0, src, stride))
    table = hip.device_table(items)
    hip.check(L.ssr_wgrad_reduce(table.data_ptr(), len(items), max(n for n, _ in shapes), hip.stream_ptr()), "ssr_wgrad_reduce")
    for (n, parts), (gd, gs, dst0, src, stride) in zip(shapes, bufs):
        s = dst0.numpy().copy()
        for p in range(parts):
            s = s + src.numpy()[p * stride:p * stride + n]          # float32 + float32, one rounding each, in part order
        assert same_bits(gd.t, torch.from_numpy(s)), (n, parts)
        assert same_bits(gs.t, src) and gd.margins_intact() and gs.margins_intact()
    assert L.ssr_wgrad_reduce(table.data_ptr(), len(items), 0, hip.stream_ptr()) == EINVAL


# ================================================================================================ ssr_split_bf16, ssr_split_bf16_multi
def _split_inputs(n, seed):
    """random values over 1e-30 .. 1e30 with the special cases in front: +-0, fp32 subnormals, ties (x exactly between two bf16 values,
    with an even and an odd upper half: round to nearest EVEN goes down resp. up), values whose hi rounds up into the next binade.
    No Inf / NaN and nothing within a bf16 ulp of FLT_MAX: the header makes no promise there."""
    g = torch.Generator().manual_seed(seed)
    x = 10 ** (torch.rand(n, generator=g).double() * 60 - 30)
    x = (x * (1 + torch.rand(n, generator=g).double())).float() * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    special = torch.tensor([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00012345, 0x007FFFFF, 0x00800000,     # zeros, subnormals, least normal
                            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x42FE8000, 0x00018000, 0x00008000,     # ties
                            0x3FFFC000, 0x3FFFFFFF, 0xBFFF8000, 0x407FFFFF, 0x7EFFC000, 0x007FC000],                # hi rounds into the next binade
                           dtype=torch.int64)
    special = (special - (special >= 2 ** 31) * 2 ** 32).to(torch.int32).view(torch.float32)
    k = min(n, special.numel())
    x[:k] = special[:k]
    return x


def _split_reference(x):
    hi = x.to(torch.bfloat16)                                       # torch CPU: round to nearest even
    lo = (x - hi.float()).to(torch.bfloat16)                        # (x - hi is exact in fp32)
    return hi, lo


def _split_check(x, hi_dev, lo_dev, tag):
    hi, lo = _split_reference(x)
    assert same_bits(hi_dev, hi), tag
    assert same_bits(lo_dev, lo), tag
    # two 8-bit pieces: |x - hi - lo| <= 2^-16 |x| (lo's rounding: half an ulp of a value of at most 2^-8 |x| ... 2^-9 |x| 2^-8); below
    # 2^-110 the lo piece is a bf16 subnormal and the floor is half their spacing, 2^-134
    res = (x.double() - hi_dev.cpu().double() - lo_dev.cpu().double()).abs()
    bound = torch.maximum(x.double().abs() * 2.0 ** -16, torch.tensor(2.0 ** -134, dtype=torch.float64))
    assert bool((res <= bound).all()), tag
    return float((res / x.double().abs().clamp_min(2.0 ** -110)).max())


@pytest.mark.parametrize("n", [4, 100004, past_cap(SPLIT_PER_BLOCK, SPLIT_CAP, 4)])
def test_split_bf16_single(n):
    """hi = bf16(x), lo = bf16(x - hi) bit for bit against torch's conversions, n = 4 (the smallest), a ragged multiple of 4 and the
    first size past the 8192-block cap.  Inputs hold no Inf / NaN and nothing within a bf16 ulp of FLT_MAX (hi would round to Inf):
    the header makes no promise there."""
    hip, L = _hip()
    x = _split_inputs(n, n)
    gx, ghi, glo = guarded_from(x), Guarded(n, torch.bfloat16), Guarded(n, torch.bfloat16)
    hip.check(L.ssr_split_bf16(gx.ptr(), ghi.ptr(), glo.ptr(), n, hip.stream_ptr()), "ssr_split_bf16")
    r = _split_check(x, ghi.t, glo.t, n)
    note("split_bf16_single", f"n={n}: max |x - hi - lo| / |x|", r, 2.0 ** -16)
    assert same_bits(gx.t, x) and ghi.margins_intact() and glo.margins_intact()
    for bad in (n + 1, n + 2, n + 3, 0):
        assert L.ssr_split_bf16(gx.ptr(), ghi.ptr(), glo.ptr(), bad, hip.stream_ptr()) == EINVAL


def test_split_bf16_multi_matches_the_single_form():
    """a table of items with n % 8 == 0 and very different n: max_n exceeds most items, the largest passes the 2048-block cap"""
    hip, L = _hip()
    ns = [8, 8008, past_cap(MULTI_PER_BLOCK, MULTI_CAP, 8), 100008, 16]
    bufs, items = [], []
    for i, n in enumerate(ns):
        x = _split_inputs(n, 100 + i)
        gx, ghi, glo = guarded_from(x), Guarded(n, torch.bfloat16), Guarded(n, torch.bfloat16)
        items.append(hip.SplitItem(gx.ptr(), ghi.ptr(), glo.ptr(), n))
        bufs.append((x, gx, ghi, glo))
    table = hip.device_table(items)
    hip.check(L.ssr_split_bf16_multi(table.data_ptr(), len(items), max(ns), hip.stream_ptr()), "ssr_split_bf16_multi")
    for n, (x, gx, ghi, glo) in zip(ns, bufs):
        _split_check(x, ghi.t, glo.t, n)
        assert same_bits(gx.t, x) and ghi.margins_intact() and glo.margins_intact()
        shi, slo = Guarded(n, torch.bfloat16), Guarded(n, torch.bfloat16)
        hip.check(L.ssr_split_bf16(gx.ptr(), shi.ptr(), slo.ptr(), n, hip.stream_ptr()), "ssr_split_bf16")
        assert same_bits(shi.t, ghi.t) and same_bits(slo.t, glo.t)              # both forms: the same bits


# ================================================================================================ ssr_axpby_f32
def _axpby(a, x, b, y):
    hip, L = _hip()
    hip.check(L.ssr_axpby_f32(a, x.ptr(), b, y.ptr(), x.n, hip.stream_ptr()), "ssr_axpby_f32")


@pytest.mark.parametrize("n", [1, 100003, past_cap(ADAM_PER_BLOCK, ADAM_CAP)])
def test_axpby_against_float64(n):
    gen = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    for a, b in ((0.5, 0.5), (0.001, 0.999), (-1.25, 0.3)):
        gx, gy = guarded_from(x), guarded_from(y)
        _axpby(a, gx, b, gy)
        a32, b32 = float(np.float32(a)), float(np.float32(b))
        ax, by = a32 * x.double(), b32 * y.double()
        # a x, b y and their sum round once each (less where the compiler fuses a product into the sum), each at its own magnitude:
        # U (|a x| + |b y| + |a x + b y|), which is 2 U |result| = one ulp where nothing cancels
        err, ratio = within(gy.t.cpu(), ax + by, U * (ax.abs() + by.abs() + (ax + by).abs()))
        note("axpby_against_float64", f"n={n} a={a} b={b}: error / bound", ratio, 1.0)
        assert ratio <= 1.0 and same_bits(gx.t, x) and gx.margins_intact() and gy.margins_intact()
    # b == 0: y is overwritten whatever it held (NaN times 0 would be NaN: the documented reason for the branch) with fl(a x)
    gx, gy = guarded_from(x), guarded_from(torch.full((n,), float("nan")))
    _axpby(0.25, gx, 0.0, gy)
    assert same_bits(gy.t, x * 0.25) and gy.margins_intact()
    gy = guarded_from(torch.full((n,), float("nan")))
    _axpby(0.3, gx, 0.0, gy)
    assert same_bits(gy.t, torch.from_numpy((np.float32(0.3) * x.numpy()).astype(np.float32)))


def test_axpby_ema_only_call_agrees_with_the_fused_adam_ema_blend():
    """train_step._phase_ema_only: ema = (1 - decay) p + decay ema through ssr_axpby_f32, against the blend of the fused Adam + EMA launch
    on the same p and ema (zero gradient and moments: the parameters stay as they are)"""
    hip, L = _hip()
    n, decay = 100003, 0.999
    gen = torch.Generator().manual_seed(9)
    p, ema = torch.randn(n, generator=gen) * 0.05, torch.randn(n, generator=gen) * 0.05
    gp, ge_axpby, ge_fused = guarded_from(p), guarded_from(ema), guarded_from(ema)
    _axpby(1.0 - decay, gp, decay, ge_axpby)
    zeros = [guarded_from(torch.zeros(n)) for _ in range(3)]
    lr, step = guarded_from(torch.tensor([1e-4])), torch.zeros(1, dtype=torch.int32, device="cuda")
    a = hip.AdamArgs(gp.ptr(), zeros[0].ptr(), zeros[1].ptr(), zeros[2].ptr(), ge_fused.ptr(), n, lr.ptr(), step.data_ptr(),
                     0.9, 0.99, 1e-8, decay, 1.0)
    hip.check(L.ssr_adam_step(C.byref(a), hip.stream_ptr()), "ssr_adam_step")
    assert same_bits(gp.t, p)
    # both evaluate ema decay + p (1 - decay) with three roundings at most: each is within U (|ema decay| + |p (1 - decay)| + |result|) of
    # the exact value for ITS coefficients, and the coefficients of p differ: fl32(1 - decay) here, 1 - fl32(decay) in the fused kernel
    a_x, a_f, d32 = float(np.float32(1.0 - decay)), float(np.float32(1.0) - np.float32(decay)), float(np.float32(decay))
    e64, p64 = ema.double(), p.double()
    exact = e64 * d32 + p64 * a_x
    bound = 2 * U * ((e64 * d32).abs() + (p64 * a_x).abs() + exact.abs()) + abs(a_x - a_f) * p64.abs()
    err, ratio = within(ge_axpby.t.cpu(), ge_fused.t.cpu(), bound)
    ulps = int((ibits(ge_axpby.t).cpu().long() - ibits(ge_fused.t).cpu().long()).abs().max())
    note("axpby_ema_only_vs_fused", f"n={n}: difference / bound (largest difference {ulps} ulp)", ratio, 1.0)
    assert ratio <= 1.0
    assert within(ge_axpby.t.cpu(), exact, U * ((e64 * d32).abs() + (p64 * a_x).abs() + exact.abs()))[1] <= 1.0
    assert ge_axpby.margins_intact() and ge_fused.margins_intact()


# ================================================================================================ ssr_fill
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fill(dtype):
    hip, L = _hip()
    code = hip.BF16 if dtype is torch.bfloat16 else hip.F32
    for n in (0, 1, 3, 100003, past_cap(FILL_PER_BLOCK, FILL_CAP)):
        for value in (0.0, 1.5, -2.0):
            g = Guarded(max(n, 1), dtype)
            hip.check(L.ssr_fill(g.ptr(), n, code, value, hip.stream_ptr()), "ssr_fill")
            assert same_bits(g.t[:n], torch.full((n,), value, dtype=dtype)), (n, value)
            assert bool((ibits(g.t[n:]) == g.sent).all()) and g.margins_intact()          # n = 0: nothing written
    g = Guarded(8, dtype)
    assert L.ssr_fill(g.ptr(), 8, 7, 1.0, hip.stream_ptr()) == EUNSUP and L.ssr_fill(g.ptr(), -1, code, 1.0, hip.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((ibits(g.t) == g.sent).all())
    if dtype is torch.float32:                                     # the fp32-storage code of the split modes
        hip.check(L.ssr_fill(g.ptr(), 8, hip.F32X3, 1.5, hip.stream_ptr()), "ssr_fill")
        assert same_bits(g.t, torch.full((8,), 1.5)) and g.margins_intact()


# ================================================================================================ ssr_add_views
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix,nc", [(1, 1), (89, 3), (4099, 24), (past_cap(ADDV_PER_BLOCK, ADDV_CAP, 64) // 64, 64)])
def test_add_views(npix, nc, dtype):
    """dst += src over channel slices of two buffers of different width.  dst holds multiples of 1/64 below 4, src multiples of 1/512 below
    1/2: 8 significant bits each (exact in bf16), sums of at most 12 bits (exact in fp32) - so fp32 is bit-exact and bf16 is ONE rounding
    of the exact sum, ties to even included."""
    hip, L = _hip()
    code = hip.BF16 if dtype is torch.bfloat16 else hip.F32
    gen = torch.Generator().manual_seed(npix)
    d0 = torch.randint(-255, 256, (npix, nc), generator=gen).double() / 64
    s0 = torch.randint(-255, 256, (npix, nc), generator=gen).double() / 512
    (dcs, dcoff), (scs, scoff) = ((16, 8), (32, 24)) if nc <= 8 else ((rnd8(nc) + 16, 8), (rnd8(nc) + 8, 0)) if nc < 64 else ((128, 64), (72, 8))
    gd, vd = strided(d0, dcs, dcoff, dtype)
    gs, vs = strided(s0, scs, scoff, dtype)
    s_before = gs.buf.clone()
    hip.check(L.ssr_add_views(vd, vs, code, npix, nc, hip.stream_ptr()), "ssr_add_views")
    want = (d0 + s0).to(dtype)                                      # float64 sum (exact), rounded once to the storage type
    assert torch.equal(ibits(read_view(gd, dcs, dcoff, nc)), ibits(want))
    assert gd.margins_intact() and gd.channels_intact(dcs, dcoff, nc) and torch.equal(ibits(gs.buf), ibits(s_before))
    assert L.ssr_add_views(vd, vs, 7, npix, nc, hip.stream_ptr()) == EUNSUP


def rnd8(c):
    return (c + 7) // 8 * 8


# ================================================================================================ ssr_pack_weights
def _pack_specs():
    from satlas_super_resolution_amd.engine import ConvSpec as S
    return [S("c3a", 5, 3), S("c3b", 32, 24), S("c3c", 64, 160, 3, 1, False, True),          # 3x3 stride 1 (the last spectral-normalised)
            S("head", 1, 64, 3, 1, True, False, dgrad_packed=False),                         # a 1-output head, forward table only
            S("d4a", 64, 32, 4, 2, False, True),                                             # 4x4 stride 2 + SN: s2d order where the mode has it
            S("d4b", 64, 32, 4, 2, False, True, s2d=False),                                  # the same layer kept in the plain order
            S("d4c", 32, 24, 4, 2, False, True), S("d4d", 5, 3, 4, 2, False, True)]          # shapes the s2d path does not take


def _pad3(val, rows_pad, cols_pad):
    out = np.zeros((rows_pad, cols_pad, val.shape[2]), np.float32)
    out[:val.shape[0], :val.shape[1]] = val
    return out


def _expected_fwd(val, it):
    """include/ssr_hip.h: [Cin chunk][KH*KW][CoutPad][ck], Cin zero-padded; space-to-depth order (ssr_conv_desc.s2d):
    [q * nchunks + chunk][2x2 taps (dy, dx)][CoutPad][ck] with tap (ky, kx) = (2 dy + (q >> 1), 2 dx + (q & 1))"""
    kk, ck = it.KH * it.KW, it.ck_fwd
    nch = it.CinPad // ck
    full = _pad3(val.reshape(it.Cout, it.Cin, kk), it.CoutPad, it.CinPad)                   # [co][ci][tap]
    out = full.reshape(it.CoutPad, nch, ck, kk).transpose(1, 3, 0, 2)                        # [chunk][tap][co][cc]
    if it.fwd_s2d:
        o = out.reshape(nch, 2, 2, 2, 2, it.CoutPad, ck)                                     # tap = (ky, kx) = (2 dy + qy, 2 dx + qx): [chunk][dy][qy][dx][qx]
        out = o.transpose(2, 4, 0, 1, 3, 5, 6)                                               # [qy][qx][chunk][dy][dx][co][cc]
    return np.ascontiguousarray(out).reshape(-1, ck)


def _expected_dgrad(val, it):
    """csrc/misc.hip: stride 1 - Wd[chunk][tap'][o = ci][k = co] = W[co][ci][KK - 1 - tap'] (rotated by 180 degrees, transposed);
    4x4 stride 2 - the transposed convolution as four output-parity classes (py, px) of 2x2 taps (ty, tx):
    [class][chunk][tap][o][ck] with ky = py ? 2 - 2 ty : 3 - 2 ty, and the same for x"""
    kk, ck = it.KH * it.KW, it.ck_dgrad
    nch = it.CoutPadI // ck
    full = _pad3(val.reshape(it.Cout, it.Cin, kk), it.CoutPadI, it.CinPadO)                 # [k = co][o = ci][tap]
    by_chunk = full.reshape(nch, ck, it.CinPadO, kk).transpose(0, 3, 2, 1)                   # [chunk][tap][o][cc]
    if it.stride == 1:
        return np.ascontiguousarray(by_chunk[:, ::-1]).reshape(-1, ck)
    out = np.zeros((4, nch, 4, it.CinPadO, ck), np.float32)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    ky, kx = (2 - 2 * ty if py else 3 - 2 * ty), (2 - 2 * tx if px else 3 - 2 * tx)
                    out[py * 2 + px, :, ty * 2 + tx] = by_chunk[:, ky * 4 + kx]
    return out.reshape(-1, ck)


def _expected_bits(rows, code, ck):
    """the stored form of fp32 rows [.., ck]: fp32 as they are; bf16 rounded once; the split modes store a row of 16 as
    [16 x hi | 16 x lo] - bf16 pieces of the value (SSR_F32X3), fp16 pieces of 2^10 times the value (SSR_F32H) - and rows of 8 as fp32"""
    hip, _ = _hip()
    r = torch.from_numpy(rows)
    if code == hip.BF16:
        return ibits(r.to(torch.bfloat16)).reshape(-1)
    if code in (hip.F32X3, hip.F32H3) and ck == 16:
        piece = torch.bfloat16 if code == hip.F32X3 else torch.float16
        r = r * (1.0 if code == hip.F32X3 else 1024.0)
        hi = r.to(piece)
        lo = (r - hi.float()).to(piece)
        return ibits(torch.cat([hi, lo], dim=1)).reshape(-1)
    return ibits(r).reshape(-1)


def _dev_bits(buf, like):
    return buf.view(like.dtype).reshape(-1).cpu()


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3", "fp32h", "fp32f"])
def test_pack_weights_layouts_bit_for_bit(mode):
    """Every element of the forward and dgrad tables against the documented index maps: values fl(w * fl(1 / sigma)) in the storage form
    of the mode, every padding element exactly +0 - the buffers start as NaN, pack() owns every element."""
    from satlas_super_resolution_amd import engine
    hip, L = _hip()
    specs = _pack_specs()
    store = engine.ParamStore(specs, hip.dtype_code(mode))
    # the space-to-depth forward order exists in bf16 and the split modes: d4a takes it there, its twin d4b is told not to
    assert store.s2d["d4a"] == (mode not in ("fp32", "fp32f")) and not (store.s2d["d4b"] or store.s2d["d4c"] or store.s2d["d4d"])
    gen = torch.Generator().manual_seed(1)
    store.data.copy_(torch.randn(store.numel, generator=gen) * 0.1)
    sig = torch.tensor([1.7, 0.6, 2.3, 0.9, 1.1][:len(store.sn_names)])
    store.sigma.copy_(sig)
    fwd_items = store._pack_items
    bwd_items = store._pack_items_bwd if store._pack_items_bwd is not None else store._pack_items
    expect = {}
    for s, itf, itb in zip(specs, fwd_items, bwd_items):
        w = store.tensor(store.wkey(s.name)).cpu().numpy()
        inv = np.float32(1.0) / np.float32(float(sig[store.sn_names.index(s.name)])) if s.sn else np.float32(1.0)
        val = (w * inv).astype(np.float32)                          # fl(w * fl(1 / sigma))
        expect[("fwd", s.name)] = _expected_bits(_expected_fwd(val, itf), store.fwd_dtype, itf.ck_fwd)
        if s.dgrad_packed:
            expect[("dgrad", s.name)] = _expected_bits(_expected_dgrad(val, itb), store.dtype, itb.ck_dgrad)
    nan = float("nan")
    # ---- through ParamStore.pack()
    for t in list(store.packed_fwd.values()) + list(store.packed_dgrad.values()):
        t.fill_(nan)
    store.pack()
    for (kind, name), want in expect.items():
        buf = (store.packed_fwd if kind == "fwd" else store.packed_dgrad)[name]
        got = _dev_bits(buf, want)
        assert got.numel() == want.numel(), (kind, name)
        assert torch.equal(got, want), (mode, kind, name, int((got != want).sum()))
    # ---- the C ABI directly, into guarded buffers that start as the NaN sentinel
    for table_items, code, kinds in ((fwd_items, store.fwd_dtype, ("fwd", "dgrad") if bwd_items is fwd_items else ("fwd",)),
                                     (bwd_items, store.dtype, () if bwd_items is fwd_items else ("dgrad",))):
        if not kinds:
            continue
        mine, guards = [], {}
        for s, it in zip(specs, table_items):
            cp = hip.PackItem()
            C.memmove(C.byref(cp), C.byref(it), C.sizeof(hip.PackItem))
            for kind, field, bufs in (("fwd", "dst_fwd", store.packed_fwd), ("dgrad", "dst_dgrad", store.packed_dgrad)):
                if kind in kinds and getattr(it, field):
                    g = Guarded(bufs[s.name].numel(), bufs[s.name].dtype)
                    guards[(kind, s.name)] = g
                    setattr(cp, field, g.ptr())
                else:
                    setattr(cp, field, None)
            mine.append(cp)
        table = hip.device_table(mine)
        hip.check(L.ssr_pack_weights(table.data_ptr(), len(mine), code, hip.stream_ptr()), "ssr_pack_weights")
        for key, g in guards.items():
            assert torch.equal(_dev_bits(g.t, expect[key]), expect[key]), (mode, key)
            assert g.margins_intact(), (mode, key)
    assert L.ssr_pack_weights(store.pack_table.data_ptr(), len(fwd_items), 9, hip.stream_ptr()) == EUNSUP
