"""GPU: the kernels that sit around every convolution and at the plugin boundary - ssr_nchw_to_nhwc / ssr_nhwc_to_nchw, ssr_bilinear2x_fwd /
_bwd and ssr_nearest2x_bwd in every form the wrapper can pick, ssr_relu_maxpool2_fwd / _bwd, ssr_channel_affine, ssr_pack_dgrad_gather -
each called through the C ABI and held to a float64 (or integer) restatement of the reference operation (F.pixel_unshuffle,
F.interpolate and its autograd, F.max_pool2d(F.relu(.)) and its autograd), never of the kernel's code.  Conventions (unit roundoff U,
sentinel margins and sentinel channels around sliced views, sizes past the grid caps, note()) as in tests/test_gpu_support_kernels.py.

Two kinds of target:
  * exact legs - inputs on which every product and sum of the operation is an integer below 256 (exact in fp32 AND bf16, in any order,
    fused or not): compared as bit patterns;
  * random legs - normal inputs against float64, element by element, within k U of the sum of the magnitudes of the terms (k roundings
    on the longest chain).  In bf16 storage the fp32 value v the kernel rounds lies in [ref - bound, ref + bound] and rounding is
    monotonic, so the stored value must lie in [bf16(ref - bound), bf16(ref + bound)]: it IS bf16(ref) unless ref lies within the fp32
    bound of a rounding boundary, and then it may be the neighbour."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_support_helpers import _dev_bits, _expected_bits
from test_gpu_support_kernels import (EINVAL, EUNSUP, U, Guarded, _hip, _report_file, guarded_from, ibits, note,  # noqa: F401
                                      past_cap, read_view, same_bits, strided, within)

pytestmark = pytest.mark.gpu

# grid caps: (elements or 16-byte vectors per block the host sizes the grid with, cap on the blocks)
LAYOUT_PER_BLOCK, LAYOUT_CAP = 256, 4096       # csrc/misc.hip ssr_nchw_to_nhwc / ssr_nhwc_to_nchw: grid_for(total) = grid_for(total, 256, 4096)
UP2X_PER_BLOCK, UP2X_CAP = 256, 8192           # csrc/misc.hip ssr_bilinear2x_fwd, up2x_bwd (per-pixel kernels): grid_for(total, 256, 8192), one vector per thread
VGG_PER_BLOCK, VGG_CAP = 256, 8192             # csrc/vgg.hip grid_of(total): g = (total + 255) / 256 capped at 8192 (pool: vectors, affine: elements)

DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]


def _code(dtype):
    hip, _ = _hip()
    return hip.BF16 if dtype is torch.bfloat16 else hip.F32


def _vec(dtype):
    return 8 if dtype is torch.bfloat16 else 4                     # elements of a 16-byte vector


def _out(npix, nc, cs, coff, dtype):
    """an output view: channels [coff, coff + nc) of a guarded [npix, cs] buffer, every element the sentinel"""
    g, v = strided(torch.zeros(npix, nc, dtype=torch.float64), cs, coff, dtype)
    ibits(g.t).fill_(g.sent)
    return g, v


def _nhwc(t):
    """[N, C, H, W] -> [N H W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(rows, N, H, W):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _bf16_round64(x):
    """float64 -> the nearest bf16 value (ties to even), computed in float64 without an fp32 step in between (normal range)"""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def _held(got, ref, bound, dtype):
    """every element of `got` against float64 `ref` and the fp32 `bound` (see the module docstring): (observed, allowed) for note().
    fp32: the largest error / bound.  bf16: the number of elements that are not bf16(ref), against the number that may be."""
    ref, bound = ref.double(), (bound.double() if torch.is_tensor(bound) else torch.full_like(ref.double(), bound))
    assert got.shape == ref.shape
    if dtype is torch.float32:
        _, ratio = within(got, ref, bound)
        assert ratio <= 1.0, ratio
        return ratio, 1.0
    g = got.double().numpy()
    assert np.isfinite(g).all()
    lo, hi = _bf16_round64((ref - bound).numpy()), _bf16_round64((ref + bound).numpy())
    assert ((g >= lo) & (g <= hi)).all(), int(((g < lo) | (g > hi)).sum())
    return float((g != _bf16_round64(ref.numpy())).sum()), float((lo != hi).sum())


def _bits_equal_nan_aware(got, want):
    """bit patterns equal; where the target is NaN the result only has to be a NaN"""
    nan = torch.isnan(want.float())
    return torch.equal(torch.isnan(got.float()), nan) and torch.equal(ibits(got)[~nan], ibits(want)[~nan])


# ================================================================================================ ssr_nchw_to_nhwc / ssr_nhwc_to_nchw
def _layout_input(shape, seed):
    """normal values with the special cases in front: +-0, fp32 subnormals, bf16 ties (even and odd upper half), +-Inf, NaN"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 10 ** torch.randint(-3, 4, shape, generator=g).float()
    sp = torch.tensor([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x3F808000, 0x3F818000, 0xBF808000,
                       0xBF818000, 0x42FE8000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF], dtype=torch.int64)
    sp = (sp - (sp >= 2 ** 31) * 2 ** 32).to(torch.int32).view(torch.float32)
    flat = x.reshape(-1)
    k = min(flat.numel(), sp.numel())
    flat[:k] = sp[:k]
    flat[-1] = sp[k - 1] if flat.numel() > 1 else flat[-1]         # and one special value at the very end
    return flat.reshape(shape)


def _to_nhwc_reference(x, s, up, scale, dtype):
    """one fp32 product (numpy), gathered by F.pixel_unshuffle and floor(o / up), one conversion to the storage type (torch)"""
    with np.errstate(all="ignore"):
        v = torch.from_numpy(x.numpy() * np.float32(scale))
    assert v.dtype == torch.float32
    v = F.pixel_unshuffle(v, s) if s > 1 else v
    H2, W2 = v.shape[2] * up, v.shape[3] * up
    v = v[:, :, torch.arange(H2) // up][:, :, :, torch.arange(W2) // up]
    return _nhwc(v).to(dtype)


def _to_nhwc(x, s, up, scale, dtype, cs_extra, coff, code=None):
    hip, L = _hip()
    N, Cc, H, W = x.shape
    C2, npix = Cc * s * s, N * (H // s * up) * (W // s * up)
    gs = guarded_from(x)
    before = gs.buf.clone()
    gd, vd = _out(npix, C2, C2 + cs_extra, coff, dtype)
    hip.check(L.ssr_nchw_to_nhwc(gs.ptr(), N, Cc, H, W, vd, _code(dtype) if code is None else code, s, up, scale, hip.stream_ptr()), "ssr_nchw_to_nhwc")
    assert gd.margins_intact() and gd.channels_intact(C2 + cs_extra, coff, C2) and torch.equal(ibits(gs.buf), ibits(before))
    return read_view(gd, C2 + cs_extra, coff, C2)


@pytest.mark.parametrize("up", [1, 2, 4])
@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_nchw_to_nhwc_bit_exact(dtype, s, up):
    sizes = [(6, 10), (12, 20)] if s < 4 else [(12, 20), (8, 4)]
    for N in (1, 3):
        for Cc in (1, 3, 5, 24):
            for H, W in sizes:
                x = _layout_input((N, Cc, H, W), 1000 * N + 10 * Cc + H)
                for scale in (1.0, 1.0 / 255, 3.0):
                    want = _to_nhwc_reference(x, s, up, scale, dtype)
                    for cs_extra, coff in ((0, 0), (11, 5)):
                        got = _to_nhwc(x, s, up, scale, dtype, cs_extra, coff)
                        assert _bits_equal_nan_aware(got, want), (N, Cc, H, W, scale, coff)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_nchw_to_nhwc_past_the_cap_and_codes(dtype):
    """17 x 61681 = 4096 * 256 + 1 elements: the first count at which a thread runs a second trip of the grid-stride loop"""
    hip, L = _hip()
    H, W = 17, 61681
    assert H * W == past_cap(LAYOUT_PER_BLOCK, LAYOUT_CAP)
    x = _layout_input((1, 1, H, W), 3)
    got = _to_nhwc(x, 1, 1, 1.0 / 255, dtype, 0, 0)
    assert _bits_equal_nan_aware(got, _to_nhwc_reference(x, 1, 1, 1.0 / 255, dtype))
    x = _layout_input((2, 3, 6, 10), 4)
    if dtype is torch.float32:                                      # the fp32-storage alias: the same bytes
        a, b = _to_nhwc(x, 2, 2, 3.0, dtype, 11, 5), _to_nhwc(x, 2, 2, 3.0, dtype, 11, 5, code=hip.F32X3)
        assert _bits_equal_nan_aware(b, a) and _bits_equal_nan_aware(a, _to_nhwc_reference(x, 2, 2, 3.0, dtype))
    # return codes, each before a launch: nothing is written
    gs = guarded_from(x)
    gd, vd = _out(2 * 6 * 10, 3 * 16, 48, 0, dtype)
    st = hip.stream_ptr()
    assert L.ssr_nchw_to_nhwc(gs.ptr(), 2, 3, 6, 10, vd, _code(dtype), 4, 1, 1.0, st) == EINVAL        # H % unshuffle != 0
    assert L.ssr_nchw_to_nhwc(gs.ptr(), 2, 3, 6, 10, vd, _code(dtype), 0, 1, 1.0, st) == EINVAL
    assert L.ssr_nchw_to_nhwc(gs.ptr(), 2, 3, 6, 10, vd, _code(dtype), 1, 0, 1.0, st) == EINVAL
    for code in (hip.F32H3, 7):
        assert L.ssr_nchw_to_nhwc(gs.ptr(), 2, 3, 6, 10, vd, code, 1, 1, 1.0, st) == EUNSUP
        assert L.ssr_nhwc_to_nchw(vd, code, gs.ptr(), 2, 3, 6, 10, st) == EUNSUP
    torch.cuda.synchronize()
    assert bool((ibits(gd.t) == gd.sent).all()) and same_bits(gs.t, x.reshape(-1))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_nhwc_to_nchw_overwrites_bit_exact(dtype):
    hip, L = _hip()
    shapes = [(1, 1, 1, 1), (1, 3, 6, 10), (3, 5, 12, 20), (3, 24, 6, 10), (1, 1, 17, 61681)]              # the last: past the 4096-block cap
    for N, Cc, H, W in shapes:
        x = _layout_input((N, Cc, H, W), N + Cc + H).to(dtype)                                              # exact in the storage type
        for cs, coff in ((Cc, 0), (Cc + 11, 5)):
            gsrc, vsrc = strided(_nhwc(x.float()), cs, coff, dtype)
            before = gsrc.buf.clone()
            gd = guarded_from(torch.full((N * Cc * H * W,), 7.5))                                          # a non-zero dst: the call overwrites
            codes = [_code(dtype)] + ([hip.F32X3] if dtype is torch.float32 and H == 6 else [])
            for code in codes:
                hip.check(L.ssr_nhwc_to_nchw(vsrc, code, gd.ptr(), N, Cc, H, W, hip.stream_ptr()), "ssr_nhwc_to_nchw")
                assert _bits_equal_nan_aware(gd.t.cpu(), x.float().reshape(-1)), (N, Cc, H, W, coff)
                assert gd.margins_intact() and torch.equal(ibits(gsrc.buf), ibits(before))
    # the only tie between the two kernels: one round trip gives the input back
    x = _layout_input((3, 5, 12, 20), 77)
    x = x.to(dtype).float()
    rows = _to_nhwc(x, 1, 1, 1.0, dtype, 11, 5)
    gsrc, vsrc = strided(rows.float(), 24, 8, dtype)
    gd = guarded_from(torch.full((x.numel(),), 7.5))
    hip.check(L.ssr_nhwc_to_nchw(vsrc, _code(dtype), gd.ptr(), 3, 5, 12, 20, hip.stream_ptr()), "ssr_nhwc_to_nchw")
    assert _bits_equal_nan_aware(gd.t.cpu(), x.reshape(-1)) and gd.margins_intact()


# ================================================================================================ bilinear x2 forward / backward, nearest x2 backward
# every form the wrapper can pick: (dtype, C, SSR_BILINEAR_FLAT OR-ed in).  C a multiple of 32 (fp32) / 64 (bf16) takes the LDS-tile kernels
UP_FORMS = [(torch.float32, 8, 0), (torch.float32, 24, 0), (torch.float32, 32, 0), (torch.float32, 96, 0), (torch.float32, 32, 1), (torch.float32, 96, 1),
            (torch.bfloat16, 8, 0), (torch.bfloat16, 24, 0), (torch.bfloat16, 64, 0), (torch.bfloat16, 192, 0), (torch.bfloat16, 64, 1), (torch.bfloat16, 192, 1)]
UP_IDS = [f"{'bf16' if d is torch.bfloat16 else 'fp32'}-C{c}{'-flat' if f else ''}" for d, c, f in UP_FORMS]
# 1x1, a single row and column, exactly one tile of the forward (4 x 16) and of the backward (4 x 8) LDS kernels, one tile plus one
# pixel in each direction, and a ragged 7 x 21
UP_GRIDS = [(1, 1), (1, 9), (9, 1), (4, 16), (4, 8), (5, 17), (5, 9), (7, 21)]
# (N, sliced): dense views of one image, and every view a channel slice of its own wider buffer for three images
UP_LAYOUTS = [(1, False), (3, True)]
# channel stride - C and channel offset of a, b, y (forward) and dy, r, y1, y, m (backward) when sliced: multiples of 8, all different
FWD_SLICES = {"a": (16, 8), "b": (8, 0), "y": (24, 16)}
BWD_SLICES = {"dy": (16, 8), "r": (8, 0), "y1": (24, 16), "y": (8, 8), "m": (16, 0)}
SLOPE32 = float(np.float32(0.2))                                   # LeakyReLU(0.2) as an fp32 network holds it


def _interp(x, mode):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False) if mode == "bilinear" else F.interpolate(x, scale_factor=2, mode="nearest")


def _adjoint(dy, mode):
    """the autograd backward of the x2 interpolation: [N, C, 2H, 2W] -> [N, C, H, W]"""
    N, Cc, H2, W2 = dy.shape
    x = torch.zeros(N, Cc, H2 // 2, W2 // 2, dtype=dy.dtype, requires_grad=True)
    return torch.autograd.grad(_interp(x, mode), x, dy)[0]


def _ints(shape, lo, hi, step, gen, dtype=torch.float64):
    return (torch.randint(lo, hi + 1, shape, generator=gen) * step).to(dtype)


def _view_in(x_nchw, Cc, sl, sliced, dtype):
    """an input tensor as a view (dense or channels of a wider guarded buffer): (Guarded, view, snapshot)"""
    extra, coff = sl if sliced else (0, 0)
    g, v = strided(_nhwc(x_nchw), Cc + extra, coff, dtype)
    return g, v, g.buf.clone()


def _fwd_call(a, b, dtype, flat, sliced, code=None):
    """ssr_bilinear2x_fwd on NCHW tensors exact in `dtype` (b may be None): the output rows [N 2H 2W, C], everything else asserted here"""
    hip, L = _hip()
    N, Cc, H, W = a.shape
    ga, va, a0 = _view_in(a, Cc, FWD_SLICES["a"], sliced, dtype)
    gb, vb, b0 = _view_in(b, Cc, FWD_SLICES["b"], sliced, dtype) if b is not None else (None, hip.NULL_VIEW, None)
    extra, coff = FWD_SLICES["y"] if sliced else (0, 0)
    gy, vy = _out(N * 4 * H * W, Cc, Cc + extra, coff, dtype)
    code = (_code(dtype) if code is None else code) | (hip.BILINEAR_FLAT if flat else 0)
    hip.check(L.ssr_bilinear2x_fwd(va, vb, vy, code, N, H, W, Cc, hip.stream_ptr()), "ssr_bilinear2x_fwd")
    assert gy.margins_intact() and gy.channels_intact(Cc + extra, coff, Cc)
    assert torch.equal(ibits(ga.buf), ibits(a0)) and (gb is None or torch.equal(ibits(gb.buf), ibits(b0)))
    return read_view(gy, Cc + extra, coff, Cc)


@pytest.mark.parametrize("dtype,Cc,flat", UP_FORMS, ids=UP_IDS)
def test_bilinear2x_fwd_exact(dtype, Cc, flat):
    """a, b in 16 {-2 .. 2}: every weight is n / 16, so every product and sum is an integer of at most 64 - y as bit patterns against
    float64 F.interpolate"""
    hip, _ = _hip()
    for H, W in UP_GRIDS:
        for N, sliced in UP_LAYOUTS:
            gen = torch.Generator().manual_seed(100 * H + W + N)
            a, b = _ints((N, Cc, H, W), -2, 2, 16, gen), _ints((N, Cc, H, W), -2, 2, 16, gen)
            for bb in (b, None):
                ref = _interp(a + bb if bb is not None else a, "bilinear")
                assert float(ref.abs().max()) <= 64 and bool((ref == ref.round()).all())
                got = _fwd_call(a, bb, dtype, flat, sliced)
                assert torch.equal(ibits(got), ibits(_nhwc(ref).to(dtype))), (H, W, N, sliced, bb is None)
    if dtype is torch.float32:                                      # the fp32-storage alias: the same bytes
        assert same_bits(_fwd_call(a, b, dtype, flat, True, code=hip.F32X3), _fwd_call(a, b, dtype, flat, True))


@pytest.mark.parametrize("dtype,Cc,flat", UP_FORMS, ids=UP_IDS)
def test_bilinear2x_fwd_random(dtype, Cc, flat):
    """normal inputs against float64, every element.  A term w_y w_x (a + b) of an output passes the fp32 sum a + b, the inner product
    and sum, the outer product and sum: 5 roundings on the longest chain, each of a partial result no larger than the interpolation of
    |a + b| - bound 5 U interp(|a + b|) (fewer roundings where the compiler fuses a product into a sum)"""
    worst = (0.0, 1.0)
    for H, W in UP_GRIDS:
        for N, sliced in UP_LAYOUTS:
            gen = torch.Generator().manual_seed(100 * H + W + N)
            a = torch.randn(N, Cc, H, W, generator=gen).to(dtype).double()
            b = torch.randn(N, Cc, H, W, generator=gen).to(dtype).double()
            for bb in (b, None):
                t = a + bb if bb is not None else a
                obs = _held(_fwd_call(a, bb, dtype, flat, sliced), _nhwc(_interp(t, "bilinear")), 5 * U * _nhwc(_interp(t.abs(), "bilinear")), dtype)
                worst = max(worst, obs, key=lambda o: o[0] / max(o[1], 1e-300))
    what = "error / bound" if dtype is torch.float32 else "elements that are not bf16(f64) / that may differ"
    note("bilinear2x_fwd_random", f"{dtype} C={Cc} flat={flat}: {what}", *worst)


# the epilogue variants: which of r, y1, y, m are given
BWD_VARIANTS = [dict(r=1, y1=1, y=1, m=1), dict(r=1, y1=1, y=0, m=0), dict(r=1, y1=0, y=1, m=0), dict(r=0, y1=0, y=1, m=1), dict(r=0, y1=1, y=1, m=0)]


def _bwd_call(fn, dy, r, m, var, dtype, flat, sliced, code=None):
    """ssr_bilinear2x_bwd / ssr_nearest2x_bwd (fn) on NCHW tensors exact in `dtype`: (y1 rows or None, y rows or None)"""
    hip, L = _hip()
    N, Cc, H2, W2 = dy.shape
    npix = N * (H2 // 2) * (W2 // 2)
    ins = [_view_in(dy, Cc, BWD_SLICES["dy"], sliced, dtype)]
    vr = vm = hip.NULL_VIEW
    if var["r"]:
        ins.append(_view_in(r, Cc, BWD_SLICES["r"], sliced, dtype))
        vr = ins[-1][1]
    if var["m"]:
        ins.append(_view_in(m, Cc, BWD_SLICES["m"], sliced, dtype))
        vm = ins[-1][1]
    outs, views = {}, {"y1": hip.NULL_VIEW, "y": hip.NULL_VIEW}
    for key in ("y1", "y"):
        if var[key]:
            extra, coff = BWD_SLICES[key] if sliced else (0, 0)
            outs[key] = (_out(npix, Cc, Cc + extra, coff, dtype), Cc + extra, coff)
            views[key] = outs[key][0][1]
    code = (_code(dtype) if code is None else code) | (hip.BILINEAR_FLAT if flat else 0)
    hip.check(getattr(L, fn)(ins[0][1], vr, views["y1"], views["y"], vm, code, N, H2 // 2, W2 // 2, Cc, hip.stream_ptr()), fn)
    res = {}
    for key, ((g, _), cs, coff) in outs.items():
        assert g.margins_intact() and g.channels_intact(cs, coff, Cc), key
        res[key] = read_view(g, cs, coff, Cc)
    for g, _, snap in ins:
        assert torch.equal(ibits(g.buf), ibits(snap))
    return res.get("y1"), res.get("y")


def _mask_values(shape, gen):
    """LeakyReLU outputs as the mask operand: +0, -0, negative and positive values, exact in bf16"""
    vals = torch.tensor([0.0, -0.0, -1.5, -0.25, 0.5, 2.0, -3.0, 0.125], dtype=torch.float64)
    return vals[torch.randint(0, vals.numel(), shape, generator=gen)]


BWD_FNS = [("ssr_bilinear2x_bwd", "bilinear"), ("ssr_nearest2x_bwd", "nearest")]


# ssr_nearest2x_bwd has per-pixel kernels only: the flag changes nothing there, one run per (dtype, C) is enough
BWD_CASES = [(fn, mode) + f for fn, mode in BWD_FNS for f in UP_FORMS if mode == "bilinear" or not f[2]]
BWD_IDS = [f"{mode}-{'bf16' if d is torch.bfloat16 else 'fp32'}-C{c}{'-flat' if f else ''}" for _, mode, d, c, f in BWD_CASES]


def _bwd_exact_targets(dy, r, m, var, mode, dtype):
    """dy in 16 {-3 .. 3}, r integer: the adjoint and s1 = adjoint + r are integers below 256 - exact.  y = s1 where m > 0, else the ONE
    product fl32(s1 * 0.2f) (numpy fp32), rounded to the storage type by torch"""
    s1 = _adjoint(dy, mode) + (r if var["r"] else 0)
    assert float(s1.abs().max()) < 256 and bool((s1 == s1.round()).all())
    y = s1
    if var["m"]:
        prod = torch.from_numpy(s1.float().numpy() * np.float32(0.2))
        assert prod.dtype == torch.float32
        y = torch.where(m > 0, s1.float(), prod)
    return _nhwc(s1).to(dtype), _nhwc(y).to(dtype)


@pytest.mark.parametrize("fn,mode,dtype,Cc,flat", BWD_CASES, ids=BWD_IDS)
def test_up2x_bwd_exact(fn, mode, dtype, Cc, flat):
    hip, _ = _hip()
    for H, W in UP_GRIDS:
        for N, sliced in UP_LAYOUTS:
            gen = torch.Generator().manual_seed(100 * H + W + N)
            dy, r = _ints((N, Cc, 2 * H, 2 * W), -3, 3, 16, gen), _ints((N, Cc, H, W), -8, 8, 1, gen)
            m = _mask_values((N, Cc, H, W), gen)
            for var in BWD_VARIANTS:
                want_y1, want_y = _bwd_exact_targets(dy, r, m, var, mode, dtype)
                y1, y = _bwd_call(fn, dy, r, m, var, dtype, flat, sliced)
                assert (y1 is None) == (not var["y1"]) and (y is None) == (not var["y"])
                if y1 is not None:
                    assert torch.equal(ibits(y1), ibits(want_y1)), (H, W, N, sliced, var)
                if y is not None:
                    assert torch.equal(ibits(y), ibits(want_y)), (H, W, N, sliced, var)
    if dtype is torch.float32:                                      # the fp32-storage alias: the same bytes
        y1x, yx = _bwd_call(fn, dy, r, m, BWD_VARIANTS[0], dtype, flat, True, code=hip.F32X3)
        y1f, yf = _bwd_call(fn, dy, r, m, BWD_VARIANTS[0], dtype, flat, True)
        assert same_bits(y1x, y1f) and same_bits(yx, yf)


@pytest.mark.parametrize("fn,mode,dtype,Cc,flat", BWD_CASES, ids=BWD_IDS)
def test_up2x_bwd_random(fn, mode, dtype, Cc, flat):
    """normal inputs against float64, every element.  With A = the adjoint applied to |dy| (the sum of the magnitudes of the terms):
    bilinear - a term passes the inner product and at most 3 inner sums, the outer product and at most 3 outer sums (the first sum of
    each, onto 0, is exact): 8 roundings; nearest - 3 sums.  Then + r (one more, of a value of at most A + |r|) gives y1, and the product
    with the slope (one more) gives y:  y1 within (k + 1) U (A + |r|), y within (k + 2) U (A + |r|) slope, k = 8 | 3."""
    k = 8 if mode == "bilinear" else 3
    worst = (0.0, 1.0)
    for H, W in UP_GRIDS:
        for N, sliced in UP_LAYOUTS:
            gen = torch.Generator().manual_seed(100 * H + W + N)
            dy = torch.randn(N, Cc, 2 * H, 2 * W, generator=gen).to(dtype).double()
            r = torch.randn(N, Cc, H, W, generator=gen).to(dtype).double()
            m = torch.randn(N, Cc, H, W, generator=gen).to(dtype).double()
            m.view(-1)[::7] = 0.0
            m.view(-1)[3::7] = -0.0
            s0, A = _adjoint(dy, mode), _adjoint(dy.abs(), mode)
            for var in BWD_VARIANTS:
                s1 = s0 + (r if var["r"] else 0)
                mag = A + (r.abs() if var["r"] else 0)
                slope = torch.where(m > 0, 1.0, SLOPE32).double() if var["m"] else torch.ones_like(s1)
                y1, y = _bwd_call(fn, dy, r, m, var, dtype, flat, sliced)
                if y1 is not None:
                    worst = max(worst, _held(y1, _nhwc(s1), (k + 1) * U * _nhwc(mag), dtype), key=lambda o: o[0] / max(o[1], 1e-300))
                if y is not None:
                    worst = max(worst, _held(y, _nhwc(s1 * slope), (k + 2) * U * _nhwc(mag * slope), dtype), key=lambda o: o[0] / max(o[1], 1e-300))
    what = "error / bound" if dtype is torch.float32 else "elements that are not bf16(f64) / that may differ"
    note(f"up2x_bwd_random[{mode}]", f"{dtype} C={Cc} flat={flat}: {what}", *worst)


def _past_cap_hw(dtype):
    """C = 8, N = 1: the smallest H x W whose vector count H W (8 / V) passes 8192 * 256"""
    H, W = (17, 61681) if dtype is torch.float32 else (3, 699051)
    assert H * W * 8 // _vec(dtype) == past_cap(UP2X_PER_BLOCK, UP2X_CAP, 8 // _vec(dtype))
    return H, W


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bilinear2x_fwd_past_the_cap(dtype):
    """the exact leg, where no tolerance can hide an index that wrapped.  The target is evaluated in float32: on these inputs every
    product and sum is an integer below 256, so the float32 evaluation is the float64 value (asserted on the first rows)"""
    H, W = _past_cap_hw(dtype)
    gen = torch.Generator().manual_seed(H)
    a, b = _ints((1, 8, H, W), -2, 2, 16, gen, torch.float32), _ints((1, 8, H, W), -2, 2, 16, gen, torch.float32)
    ref = _interp(a + b, "bilinear")
    assert torch.equal(ref[..., :4000].double(), _interp((a + b)[..., :2048].double(), "bilinear")[..., :4000])
    got = _fwd_call(a, b, dtype, 0, False)
    assert torch.equal(ibits(got), ibits(_nhwc(ref).to(dtype)))


@pytest.mark.parametrize("fn,mode", BWD_FNS, ids=["bilinear", "nearest"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_up2x_bwd_past_the_cap(dtype, fn, mode):
    H, W = _past_cap_hw(dtype)
    gen = torch.Generator().manual_seed(H)
    dy, r = _ints((1, 8, 2 * H, 2 * W), -3, 3, 16, gen, torch.float32), _ints((1, 8, H, W), -8, 8, 1, gen, torch.float32)
    m = _mask_values((1, 8, H, W), gen).float()
    want_y1, want_y = _bwd_exact_targets(dy, r, m, BWD_VARIANTS[0], mode, dtype)
    small = _bwd_exact_targets(dy[..., :512].double(), r[..., :256].double(), m[..., :256].double(), BWD_VARIANTS[0], mode, dtype)
    assert torch.equal(_nchw(want_y, 1, H, W)[..., :250], _nchw(small[1], 1, H, 256)[..., :250])        # float32 evaluation = float64 on these inputs
    y1, y = _bwd_call(fn, dy, r, m, BWD_VARIANTS[0], dtype, 0, False)
    assert torch.equal(ibits(y1), ibits(want_y1)) and torch.equal(ibits(y), ibits(want_y))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_up2x_return_codes_before_any_launch(dtype):
    hip, L = _hip()
    N, H, W, Cc = 1, 3, 5, 16
    st, code = hip.stream_ptr(), _code(dtype)
    zeros = torch.zeros(N * H * W, 24, dtype=torch.float64)
    gi, vi = strided(zeros, 24, 0, dtype)                           # inputs (a, b, r, m)
    gd, vdy = strided(torch.zeros(N * 4 * H * W, 24, dtype=torch.float64), 24, 0, dtype)
    go, vo = _out(N * 4 * H * W, 16, 24, 0, dtype)                  # outputs (large enough for y of the forward)

    def view(g, cs, coff):
        return hip.View(g.ptr(), cs, coff)
    # forward
    assert L.ssr_bilinear2x_fwd(vi, hip.NULL_VIEW, vo, code, N, H, W, 4, st) == EINVAL                    # C = 4
    assert L.ssr_bilinear2x_fwd(view(gi, 24, 4), hip.NULL_VIEW, vo, code, N, H, W, Cc, st) == EINVAL      # a.coff = 4
    assert L.ssr_bilinear2x_fwd(vi, view(gi, 20, 0), vo, code, N, H, W, 8, st) == EINVAL
    assert L.ssr_bilinear2x_fwd(vi, hip.NULL_VIEW, view(go, 24, 4), code, N, H, W, 8, st) == EINVAL
    assert L.ssr_bilinear2x_fwd(vi, hip.NULL_VIEW, vo, 7, N, H, W, 8, st) == EUNSUP
    # backward: every view that is given goes through 16-byte vector loads / stores
    for fn in (L.ssr_bilinear2x_bwd, L.ssr_nearest2x_bwd):
        ok = dict(dy=vdy, r=vi, y1=vo, y=view(go, 24, 8), m=view(gi, 24, 8))
        assert fn(ok["dy"], ok["r"], ok["y1"], ok["y"], ok["m"], code, N, H, W, 4, st) == EINVAL          # C = 4
        assert fn(ok["dy"], ok["r"], hip.NULL_VIEW, hip.NULL_VIEW, ok["m"], code, N, H, W, 8, st) == EINVAL   # no output at all
        for key in ("dy", "r", "y1", "y", "m"):
            g = gd if key == "dy" else go if key in ("y1", "y") else gi
            for cs, coff in ((24, 4), (20, 0), (28, 8)):
                args = dict(ok)
                args[key] = view(g, cs, coff)
                assert fn(args["dy"], args["r"], args["y1"], args["y"], args["m"], code, N, H, W, 8, st) == EINVAL, (key, cs, coff)
        assert fn(ok["dy"], ok["r"], ok["y1"], ok["y"], ok["m"], 7, N, H, W, 8, st) == EUNSUP
    torch.cuda.synchronize()
    assert bool((ibits(go.t) == go.sent).all()) and go.margins_intact()


# ================================================================================================ ssr_relu_maxpool2_fwd / _bwd
# 2x2 windows (row-major: (0,0), (0,1), (1,0), (1,1)), each laid over every channel of a vector: the maximum in each of the four positions,
# two equal positive maxima at (0,1) + (1,1) and at (1,0) + (1,1), all four equal and positive, all zero, all negative, mixed sign
# with maximum +0
POOL_WINDOWS = [(3, 1, 2, -1), (1, 3, -2, 2), (0, 1, 3, 2), (-1, 2, 1, 3), (1, 2, 0, 2), (-3, 1, 2, 2), (2, 2, 2, 2), (0, 0, 0, 0),
                (-1, -2, -3, -1), (-1, 0, -2, 0), (2, 3, 3, 1), (-0.0, 0.0, -1, -0.0)]


def _pool_input(N, Cc, H, W, gen, dtype):
    """small integers (ties in most windows), the windows above in front"""
    f = torch.randint(-2, 4, (N, Cc, H, W), generator=gen, dtype=torch.int8).to(dtype)
    for k, w in enumerate(POOL_WINDOWS[:(H // 2) * (W // 2)]):
        y, x = 2 * (k // (W // 2)), 2 * (k % (W // 2))
        f[0, :, y, x], f[0, :, y, x + 1], f[0, :, y + 1, x], f[0, :, y + 1, x + 1] = w
    return f


def _pool_reference(f, gp):
    fr = f.clone().requires_grad_(True)
    p = F.max_pool2d(F.relu(fr), 2)
    return p.detach(), torch.autograd.grad(p, fr, gp)[0]


def _pool_check(N, Cc, H, W, dtype, sliced, ref_dtype=torch.float64):
    hip, L = _hip()
    v = _vec(dtype)
    gen = torch.Generator().manual_seed(N * 1000 + Cc + H * W)
    f = _pool_input(N, Cc, H, W, gen, ref_dtype)
    gpool = torch.randint(-4, 5, (N, Cc, H // 2, W // 2), generator=gen, dtype=torch.int8).to(ref_dtype)
    pattern = torch.randint(-4, 5, (N, Cc, H, W), generator=gen, dtype=torch.int8).to(ref_dtype)
    want_p, want_g = _pool_reference(f, gpool)
    sl = {"f": (2 * v, v), "p": (v, 0), "gp": (3 * v, 2 * v), "g": (v, v)} if sliced else {k: (0, 0) for k in ("f", "p", "gp", "g")}
    gf, vf = strided(_nhwc(f), Cc + sl["f"][0], sl["f"][1], dtype)
    ggp, vgp = strided(_nhwc(gpool), Cc + sl["gp"][0], sl["gp"][1], dtype)
    f0, gp0 = gf.buf.clone(), ggp.buf.clone()
    st, code = hip.stream_ptr(), _code(dtype)
    # forward into a sentinel buffer
    gp_, vp = _out(N * (H // 2) * (W // 2), Cc, Cc + sl["p"][0], sl["p"][1], dtype)
    hip.check(L.ssr_relu_maxpool2_fwd(vf, vp, code, N, H, W, Cc, st), "ssr_relu_maxpool2_fwd")
    assert torch.equal(read_view(gp_, Cc + sl["p"][0], sl["p"][1], Cc).double(), _nhwc(want_p).double())
    assert gp_.margins_intact() and gp_.channels_intact(Cc + sl["p"][0], sl["p"][1], Cc)
    # backward: accumulate = 0 into the sentinel, accumulate = 1 onto a known pattern
    cs, coff = Cc + sl["g"][0], sl["g"][1]
    for acc in (0, 1):
        if acc:
            gg, vg = strided(_nhwc(pattern), cs, coff, dtype)
        else:
            gg, vg = _out(N * H * W, Cc, cs, coff, dtype)
        hip.check(L.ssr_relu_maxpool2_bwd(vf, vgp, vg, code, N, H, W, Cc, acc, st), "ssr_relu_maxpool2_bwd")
        want = want_g + pattern if acc else want_g
        assert torch.equal(read_view(gg, cs, coff, Cc).double(), _nhwc(want).double()), (N, Cc, H, W, sliced, acc)
        assert gg.margins_intact() and gg.channels_intact(cs, coff, Cc)
    assert torch.equal(ibits(gf.buf), ibits(f0)) and torch.equal(ibits(ggp.buf), ibits(gp0))


@pytest.mark.parametrize("sliced", [False, True], ids=["dense", "sliced"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_relu_maxpool2_against_torch(dtype, sliced):
    """by value (-0 equals +0) against F.max_pool2d(F.relu(.)) and its autograd in float64; all values are small integers, exact in
    the storage type, so the sums of accumulate = 1 are exact too"""
    hip, L = _hip()
    for N in (1, 2):
        for H, W in ((2, 2), (2, 6), (12, 20)):
            for Cc in (_vec(dtype), 24, 64):
                _pool_check(N, Cc, H, W, dtype, sliced)
    if dtype is torch.float32 and not sliced:                       # the fp32-storage alias and the return codes
        st = hip.stream_ptr()
        gf, vf = strided(torch.zeros(4 * 6, 16, dtype=torch.float64), 16, 0, dtype)
        go, vo = _out(6, 8, 16, 0, dtype)
        for code in (hip.F32, hip.BF16):
            vv = 4 if code == hip.F32 else 8
            assert L.ssr_relu_maxpool2_fwd(vf, vo, code, 1, 3, 6, 8, st) == EINVAL                         # odd H
            assert L.ssr_relu_maxpool2_fwd(vf, vo, code, 1, 4, 5, 8, st) == EINVAL                         # odd W
            assert L.ssr_relu_maxpool2_fwd(vf, vo, code, 1, 4, 6, vv + 2, st) == EINVAL                    # C no multiple of the vector
            assert L.ssr_relu_maxpool2_fwd(hip.View(gf.ptr(), 16, vv // 2), vo, code, 1, 4, 6, 8, st) == EINVAL       # coff
            assert L.ssr_relu_maxpool2_bwd(vf, vf, hip.View(go.ptr(), 16, vv // 2), code, 1, 4, 6, 8, 0, st) == EINVAL
            assert L.ssr_relu_maxpool2_bwd(vf, hip.View(gf.ptr(), 16 + vv // 2, 0), vo, code, 1, 4, 6, 8, 1, st) == EINVAL
        assert L.ssr_relu_maxpool2_fwd(vf, vo, 7, 1, 4, 6, 8, st) == EUNSUP
        torch.cuda.synchronize()
        assert bool((ibits(go.t) == go.sent).all())
        hip.check(L.ssr_relu_maxpool2_fwd(vf, vo, hip.F32X3, 1, 4, 6, 8, st), "ssr_relu_maxpool2_fwd")
        assert torch.equal(read_view(go, 16, 0, 8), torch.zeros(6, 8)) and go.channels_intact(16, 0, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_relu_maxpool2_past_the_cap(dtype):
    """C = one vector, 3 x 699051 = 8192 * 256 + 1 pooled pixels.  Every value is a small integer: the float32 evaluation of the reference
    is exact, as the float64 one is"""
    Hp, Wp = 3, 699051
    assert Hp * Wp == past_cap(VGG_PER_BLOCK, VGG_CAP)
    _pool_check(1, _vec(dtype), 2 * Hp, 2 * Wp, dtype, False, ref_dtype=torch.float32)


# ================================================================================================ ssr_channel_affine
def _affine_call(x, y0, scale, shift, acc, dtype, sl_x, sl_y, code=None):
    """x, y0: [npix, C] exact in dtype; y0 None: y starts as the sentinel"""
    hip, L = _hip()
    npix, Cc = x.shape
    gx, vx = strided(x, Cc + sl_x[0], sl_x[1], dtype)
    x0 = gx.buf.clone()
    cs, coff = Cc + sl_y[0], sl_y[1]
    gy, vy = strided(y0, cs, coff, dtype) if y0 is not None else _out(npix, Cc, cs, coff, dtype)
    sc, sh = (C.c_float * Cc)(*scale), (C.c_float * Cc)(*shift)
    hip.check(L.ssr_channel_affine(vx, vy, _code(dtype) if code is None else code, npix, Cc, sc, sh, acc, hip.stream_ptr()), "ssr_channel_affine")
    assert gy.margins_intact() and gy.channels_intact(cs, coff, Cc) and torch.equal(ibits(gx.buf), ibits(x0))
    return read_view(gy, cs, coff, Cc)


AFFINE_NPIX = {1: [1, 257, past_cap(VGG_PER_BLOCK, VGG_CAP)], 3: [1, 257, past_cap(VGG_PER_BLOCK, VGG_CAP, 3) // 3],
               8: [1, 257, past_cap(VGG_PER_BLOCK, VGG_CAP, 8) // 8]}


@pytest.mark.parametrize("Cc", [1, 3, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_channel_affine(dtype, Cc):
    hip, L = _hip()
    mean, std = (0.485, 0.456, 0.406, 0.5, 0.1, -0.3, 0.25, 1.5)[:Cc], (0.229, 0.224, 0.225, 0.3, 2.0, 0.7, 1.1, 0.05)[:Cc]
    scale = [float(np.float32(1.0 / s)) for s in std]
    shift = [float(np.float32(-m / s)) for m, s in zip(mean, std)]
    sc64, sh64 = torch.tensor(scale, dtype=torch.float64), torch.tensor(shift, dtype=torch.float64)
    worst = (0.0, 1.0)
    for npix in AFFINE_NPIX[Cc]:
        gen = torch.Generator().manual_seed(npix + Cc)
        x = torch.randn(npix, Cc, generator=gen).to(dtype).double()
        y0 = torch.randn(npix, Cc, generator=gen).to(dtype).double()
        big = npix > 257
        for sl_x, sl_y in (((0, 0), (0, 0)),) if big else (((0, 0), (0, 0)), ((5, 2), (11, 7))):
            xs = x * sc64
            # accumulate = 0: the product and the sum round once each - U |x s| + U |x s + t|; fused into one operation only the second term
            # remains, so the bound holds either way
            got = _affine_call(x, None, scale, shift, 0, dtype, sl_x, sl_y)
            worst = max(worst, _held(got, xs + sh64, U * (xs.abs() + (xs + sh64).abs()), dtype), key=lambda o: o[0] / max(o[1], 1e-300))
            # accumulate = 1 onto a preloaded y: one more rounding, of the final sum
            got = _affine_call(x, y0, scale, shift, 1, dtype, sl_x, sl_y)
            worst = max(worst, _held(got, xs + sh64 + y0, U * (xs.abs() + (xs + sh64).abs() + (xs + sh64 + y0).abs()), dtype),
                        key=lambda o: o[0] / max(o[1], 1e-300))
            # the adjoint use: shift = 0, accumulate = 1 - the product and one sum
            got = _affine_call(x, y0, scale, [0.0] * Cc, 1, dtype, sl_x, sl_y)
            worst = max(worst, _held(got, xs + y0, U * (xs.abs() + (xs + y0).abs()), dtype), key=lambda o: o[0] / max(o[1], 1e-300))
            # exact operands: scale a power of two, integer x, shift and y - integers below 256, bit for bit in both storage types
            xi = (torch.randint(-7, 8, (npix, Cc), generator=gen) * 2).double()                        # even: x / 2 is an integer too
            yi = torch.randint(-40, 41, (npix, Cc), generator=gen).double()
            p2, ti = [(4.0, 0.5, -2.0, 1.0, 8.0, -0.5, 2.0, -4.0)[c] for c in range(Cc)], [float(c - 3) for c in range(Cc)]
            want0 = xi * torch.tensor(p2, dtype=torch.float64) + torch.tensor(ti, dtype=torch.float64)
            assert float((want0.abs() + yi.abs()).max()) < 256 and bool((want0 == want0.round()).all())
            assert torch.equal(ibits(_affine_call(xi, None, p2, ti, 0, dtype, sl_x, sl_y)), ibits(want0.to(dtype)))
            assert torch.equal(ibits(_affine_call(xi, yi, p2, ti, 1, dtype, sl_x, sl_y)), ibits((want0 + yi).to(dtype)))
    what = "error / bound" if dtype is torch.float32 else "elements that are not bf16(f64) / that may differ"
    note("channel_affine", f"{dtype} C={Cc}: {what}", *worst)
    if Cc == 3:
        st = hip.stream_ptr()
        g, v = _out(4, 8, 8, 0, dtype)
        f9 = (C.c_float * 9)(*([1.0] * 9))
        assert L.ssr_channel_affine(v, v, _code(dtype), 4, 0, f9, f9, 0, st) == EINVAL
        assert L.ssr_channel_affine(v, v, _code(dtype), 4, 9, f9, f9, 0, st) == EINVAL
        assert L.ssr_channel_affine(v, v, 7, 4, 3, f9, f9, 0, st) == EUNSUP
        torch.cuda.synchronize()
        assert bool((ibits(g.t) == g.sent).all())
        if dtype is torch.float32:                                  # the fp32-storage alias: the same bytes
            a = _affine_call(x, y0, scale, shift, 1, dtype, (5, 2), (11, 7))
            assert same_bits(a, _affine_call(x, y0, scale, shift, 1, dtype, (5, 2), (11, 7), code=hip.F32X3))


# ================================================================================================ ssr_pack_dgrad_gather
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp32x3"])
def test_pack_dgrad_gather_index_map(mode):
    """include/ssr_hip.h: dst[chunk][tap'][o][cc], k = chunk ck + cc, = scale * src[k - kbase][ci0 + o][8 - tap'] for kbase <= k < kbase + Cout,
    rows o >= nci zero.  The segments of slice x3 of a dense block (nf 64, gc 32: conv4's and conv5's input channels 128 .. 159, conv5
    scaled by 0.2) gathered into one table, and a third segment with nci < rows_pad into a second; both tables one chunk longer than
    the segments' K ranges, which must stay as they were (the NaN sentinel)"""
    hip, L = _hip()
    code = hip.dtype_code(mode)
    tdt = hip.torch_dtype(code)
    ck = L.ssr_conv2d_ck(code, 3)
    assert ck in (8, 16, 32, 64)
    gen = torch.Generator().manual_seed(ck)
    rows_pad = 32
    # (table, src shape, scale, ci0, nci, kbase)
    segs = [(0, (32, 160), 1.0, 128, 32, 0), (0, (64, 192), 0.2, 128, 32, 32), (1, (32, 40), 0.04, 8, 20, 16)]
    kpad = [(96 + ck - 1) // ck * ck + ck, (48 + ck - 1) // ck * ck + ck]
    tables = [Guarded(kp * 9 * rows_pad, tdt) for kp in kpad]
    want = [np.zeros((kp // ck, 9, rows_pad, ck), np.float32) for kp in kpad]
    written = [np.zeros((kp // ck, 9, rows_pad, ck), bool) for kp in kpad]
    items, srcs = [], []
    for t, (cout, cin), scale, ci0, nci, kbase in segs:
        w = torch.randn(cout, cin, 3, 3, generator=gen) * 0.1
        gs = guarded_from(w)
        srcs.append((gs, gs.buf.clone()))
        items.append(hip.PackSeg(gs.ptr(), tables[t].ptr(), scale, cout, cin, ci0, nci, kbase, rows_pad, ck))
        val = (w.numpy() * np.float32(scale)).astype(np.float32).reshape(cout, cin, 9)      # fl32(scale * w)
        for kk in range(cout):
            k = kbase + kk
            written[t][k // ck, :, :, k % ck] = True
            # [tap'][o] = val[kk][ci0 + o][8 - tap'] for o < nci, +0 for the rows up to rows_pad
            want[t][k // ck, :, :nci, k % ck] = val[kk, ci0:ci0 + nci, ::-1].T
    table = hip.device_table(items)
    hip.check(L.ssr_pack_dgrad_gather(table.data_ptr(), len(items), code, hip.stream_ptr()), "ssr_pack_dgrad_gather")
    for t in range(2):
        bits = _expected_bits(want[t].reshape(-1, ck), code, ck)
        got = _dev_bits(tables[t].t, bits)
        sent = _dev_bits(Guarded(tables[t].n, tdt).t, bits)
        # the written flag in the stored form: the split mode stores a row of 16 values as 32 pieces, rows are written whole
        wr = torch.from_numpy(written[t].reshape(-1, ck))
        if bits.numel() == 2 * wr.numel():
            assert bool((wr.all(dim=1) | ~wr.any(dim=1)).all())
            wr = torch.cat([wr, wr], dim=1)
        wr = wr.reshape(-1)
        assert got.numel() == bits.numel() == wr.numel() and 0 < int(wr.sum()) < wr.numel()
        assert torch.equal(got[wr], bits[wr]), (mode, t, int((got[wr] != bits[wr]).sum()))
        assert torch.equal(got[~wr], sent[~wr]), (mode, t)
        assert tables[t].margins_intact()
    for gs, snap in srcs:
        assert torch.equal(ibits(gs.buf), ibits(snap))
    assert L.ssr_pack_dgrad_gather(table.data_ptr(), len(items), hip.F32H3, hip.stream_ptr()) == EUNSUP
    assert L.ssr_pack_dgrad_gather(table.data_ptr(), 0, code, hip.stream_ptr()) == EINVAL
