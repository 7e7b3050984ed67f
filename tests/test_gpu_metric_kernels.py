"""GPU: the kernels of csrc/metrics.hip - ssr_quantize_u8 (_checked), ssr_metric_shift_sums, ssr_metric_ssim_sums - and ssr_usm_sharp
(csrc/misc.hip), each called through the C ABI and held to numpy / torch restatements of the reference operation: bytes and int64 sums
as integers, the float64 SSIM sums and the fp32 USM output to bounds derived next to their assertions.  Conventions (unit roundoff,
sentinel margins, sizes past the grid caps, note()) as in tests/test_gpu_support_kernels.py."""
import functools
import math

import numpy as np
import pytest
import torch

from test_gpu_support_kernels import (EINVAL, EUNSUP, U, Guarded, _hip, _report_file, guarded_from, ibits, note,  # noqa: F401
                                      past_cap, read_view, same_bits, strided, within)

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53                                       # unit roundoff of fp64

# grid caps of csrc/metrics.hip: (elements per block the host sizes the grid with, cap on the blocks)
QUANT_PER_BLOCK, QUANT_CAP = 256, 4096                 # ssr_quantize_u8 (_checked): g = (total + 255) / 256, if (g > 4096) g = 4096
SHIFT_PER_BLOCK, SHIFT_CAP = 256 * 8, 256              # ssr_metric_shift_sums: gy = (total + 256 * 8 - 1) / (256 * 8), if (gy > 256) gy = 256
SSIM_PER_BLOCK, SSIM_CAP = 256, 1024                   # ssr_metric_ssim_sums: gx = (total + 255) / 256, if (gx > 1024) gx = 1024


def _bytes(n):
    """n bytes on the device inside a Guarded fp32 buffer (sentinel margins; the tail of the last word stays sentinel): (Guarded, uint8 view)"""
    g = Guarded((n + 3) // 4)
    return g, g.t.view(torch.uint8)


def _bytes_from(arr):
    g, b = _bytes(arr.size)
    b[:arr.size] = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1)).cuda()
    return g, b


def _tail_intact(g, b, n):
    """the sentinel margins, and the bytes of the last word past the n payload bytes"""
    want = torch.tensor([g.sent], dtype=torch.int32).view(torch.uint8).repeat((b.numel() + 3) // 4)[n:b.numel()]
    return g.margins_intact() and torch.equal(b[n:].cpu(), want)


def _words(n, dtype):
    """n 8-byte (or 4-byte) words of `dtype` between sentinel margins: (Guarded, view)"""
    k = torch.empty(0, dtype=dtype).element_size() // 4
    g = Guarded(n * k)
    return g, g.t.view(dtype)


# ================================================================================================ ssr_quantize_u8 (_checked)
def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _quant_specials():
    """what the header's clamp(0, 1) * 255, round-half-even | truncate has to get right, most important first"""
    one = np.float32(1.0)
    head = np.concatenate([
        np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32), _f32([0x7FC5A5A5, 0xFFC00001, 0x00000001, 0x80000001, 0x007FFFFF]),
        np.array([np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)), -1.0, -1e-20, 1.5, 256.0, 3e38, -3e38, 0.5], np.float32)])
    k = np.arange(256, dtype=np.float64)
    return np.concatenate([head, (k / 255).astype(np.float32), ((k[:255] + 0.5) / 255).astype(np.float32)])


def _quant_reference(x, mode):
    """numpy on the same fp32 arithmetic: clamp(0, 1), one fp32 product with 255, then rint (half to even) or truncation; NaN counts
    as 0 (numpy's cast of NaN is undefined: the kernel's fmaxf(NaN, 0) = 0 is what the header's 'NaN -> 0' states)"""
    v = np.where(np.isnan(x), np.float32(0), x).astype(np.float32)
    v = np.minimum(np.maximum(v, np.float32(0)), np.float32(1)) * np.float32(255)
    assert v.dtype == np.float32
    q = np.rint(v) if mode == 0 else np.trunc(v)
    return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))       # NCHW -> NHWC


QUANT_SHAPES = [(1, 1, 5, 7), (2, 3, 17, 23), (1, 4, 16, 33), (2, 1, 9, 31), (1, 1, 17, 61681)]      # 17 * 61681 = 4096 * 256 + 1
assert QUANT_SHAPES[-1][2] * QUANT_SHAPES[-1][3] == past_cap(QUANT_PER_BLOCK, QUANT_CAP)


@pytest.mark.parametrize("mode", [0, 1], ids=["round", "trunc"])
@pytest.mark.parametrize("shape", QUANT_SHAPES, ids=["x".join(map(str, s)) for s in QUANT_SHAPES])
def test_quantize_u8_every_byte(shape, mode):
    hip, L = _hip()
    N, Cc, H, W = shape
    total = N * Cc * H * W
    rng = np.random.default_rng(total + mode)
    x = rng.uniform(-0.2, 1.2, total).astype(np.float32)
    sp = _quant_specials()
    k = min(total, sp.size)
    x[:k] = sp[:k]
    x = x.reshape(shape)
    want = _quant_reference(x, mode)
    # the literals the reference operation gives for the non-finite samples: NaN, +Inf, -Inf are x[0], x[1], x[2] in NCHW order
    flat = want.transpose(0, 3, 1, 2).reshape(-1)
    assert flat[0] == 0 and flat[1] == 255 and flat[2] == 0 and flat[3] == 0
    if total > 20:
        assert flat[5] == 0 and flat[6] == 0 and flat[10] == (255 if mode == 0 else 254) and flat[11] == 255 and flat[12] == 255
    gs = guarded_from(torch.from_numpy(x))
    before = gs.buf.clone()
    gd, d = _bytes(total)
    hip.check(L.ssr_quantize_u8(gs.ptr(), d.data_ptr(), N, Cc, H, W, mode, hip.stream_ptr()), "ssr_quantize_u8")
    got = d[:total].cpu().numpy()
    assert np.array_equal(got, want.reshape(-1)), int((got != want.reshape(-1)).sum())
    assert _tail_intact(gd, d, total) and torch.equal(ibits(gs.buf), ibits(before))

    # ---- _checked: the same bytes, the counter rises by the number of non-finite samples planted
    nonfinite = int((~np.isfinite(x)).sum())
    assert nonfinite == (3 + 2 if total > 20 else 3)
    for preload in (0, 7):
        gc, cnt = _words(1, torch.int32)
        cnt[0] = preload
        gd2, d2 = _bytes(total)
        hip.check(L.ssr_quantize_u8_checked(gs.ptr(), d2.data_ptr(), N, Cc, H, W, mode, cnt.data_ptr(), hip.stream_ptr()), "checked")
        assert np.array_equal(d2[:total].cpu().numpy(), got) and _tail_intact(gd2, d2, total)
        assert int(cnt[0]) == preload + nonfinite and gc.margins_intact()


@pytest.mark.parametrize("shape", [(1, 3, 7, 11), (2, 3, 33, 47), (1, 1, 17, 61681)], ids=["231", "9306", "past_cap"])
def test_quantize_u8_checked_counts_what_was_planted(shape):
    """finite input: the counter stays as it is; then NaN / +-Inf in the first wave, in the last (partial) wave and in a middle block"""
    hip, L = _hip()
    N, Cc, H, W = shape
    total = N * Cc * H * W
    rng = np.random.default_rng(total)
    x = rng.uniform(-0.2, 1.2, total).astype(np.float32)
    gs = guarded_from(torch.from_numpy(x))
    gc, cnt = _words(1, torch.int32)
    cnt[0] = 7
    gd, d = _bytes(total)
    hip.check(L.ssr_quantize_u8_checked(gs.ptr(), d.data_ptr(), N, Cc, H, W, 0, cnt.data_ptr(), hip.stream_ptr()), "checked")
    assert int(cnt[0]) == 7 and gc.margins_intact()
    # the kernel walks the NHWC order e; sample e of the output is src[n][c][y][x]: plant by OUTPUT position
    where = sorted({0, 1, 63, total - 1, total - 2, total // 2, total // 2 + 1, total // 2 + 64} & set(range(total)))
    vals = [np.nan, np.inf, -np.inf]
    xe = np.ascontiguousarray(x.reshape(shape).transpose(0, 2, 3, 1)).reshape(-1)
    for i, e in enumerate(where):
        xe[e] = vals[i % 3]
    x2 = np.ascontiguousarray(xe.reshape(N, H, W, Cc).transpose(0, 3, 1, 2))
    gs2 = guarded_from(torch.from_numpy(x2))
    for mode in (0, 1):
        cnt[0] = 7
        hip.check(L.ssr_quantize_u8_checked(gs2.ptr(), d.data_ptr(), N, Cc, H, W, mode, cnt.data_ptr(), hip.stream_ptr()), "checked")
        assert int(cnt[0]) == 7 + len(where) and gc.margins_intact()
        assert np.array_equal(d[:total].cpu().numpy(), _quant_reference(x2, mode).reshape(-1)) and _tail_intact(gd, d, total)


def test_quantize_u8_return_codes():
    hip, L = _hip()
    gs = guarded_from(torch.zeros(24))
    gd, d = _bytes(24)
    gc, cnt = _words(1, torch.int32)
    st = hip.stream_ptr()
    assert L.ssr_quantize_u8(gs.ptr(), d.data_ptr(), 1, 3, 2, 4, 2, st) == EINVAL
    assert L.ssr_quantize_u8_checked(gs.ptr(), d.data_ptr(), 1, 3, 2, 4, 2, cnt.data_ptr(), st) == EINVAL
    assert L.ssr_quantize_u8_checked(gs.ptr(), d.data_ptr(), 1, 3, 2, 4, 0, None, st) == EINVAL
    assert L.ssr_quantize_u8(gs.ptr(), d.data_ptr(), 1, 0, 2, 4, 0, st) == EINVAL
    torch.cuda.synchronize()
    assert _tail_intact(gd, d, 0) and bool((ibits(gc.t) == gc.sent).all())


# ================================================================================================ ssr_metric_shift_sums
def _shift_reference(a, b, crop, m):
    """include/ssr_hip.h: out[((ro (m + 1) + co) C + c) 2 + {0, 1}] = sum d, sum d^2 over the (H - 2 crop - m) x (W - 2 crop - m) window,
    d = a[y + crop + ro][x + crop + co][c] - b[y + crop + m - ro][x + crop + m - co][c] - in numpy integers: |d| <= 255 fits int16 and
    d^2 <= 65025 fits int32 exactly; both sums are accumulated in int64"""
    H, W, Cc = a.shape
    hc, wc = H - 2 * crop - m, W - 2 * crop - m
    A, B = a.astype(np.int16), b.astype(np.int16)
    out = np.zeros((m + 1, m + 1, Cc, 2), np.int64)
    for ro in range(m + 1):
        for co in range(m + 1):
            d = A[crop + ro:crop + ro + hc, crop + co:crop + co + wc] - B[crop + m - ro:crop + m - ro + hc, crop + m - co:crop + m - co + wc]
            out[ro, co, :, 0] = d.sum(axis=(0, 1), dtype=np.int64)
            out[ro, co, :, 1] = (d.astype(np.int32) ** 2).sum(axis=(0, 1), dtype=np.int64)
    return out.reshape(-1)


def _shift_run(a, b, crop, m):
    hip, L = _hip()
    H, W, Cc = a.shape
    n_out = (m + 1) ** 2 * Cc * 2
    ga, da = _bytes_from(a)
    gb, db = _bytes_from(b)
    a0, b0 = ga.buf.clone(), gb.buf.clone()
    go, out = _words(n_out, torch.int64)
    out.fill_(0x0123456789ABCDE)                                   # the call overwrites whatever out held
    hip.check(L.ssr_metric_shift_sums(da.data_ptr(), db.data_ptr(), H, W, Cc, crop, m, out.data_ptr(), hip.stream_ptr()), "shift_sums")
    got = out.cpu().numpy().copy()
    assert go.margins_intact() and torch.equal(ibits(ga.buf), ibits(a0)) and torch.equal(ibits(gb.buf), ibits(b0))
    return got


@pytest.mark.parametrize("crop", [0, 4])
@pytest.mark.parametrize("m", [0, 1, 8, 15])
@pytest.mark.parametrize("Cc", [1, 2, 3, 4])
def test_shift_sums_are_the_integers(Cc, m, crop):
    rng = np.random.default_rng(100 * Cc + 10 * m + crop)
    side = 2 * crop + m + 1
    for H, W, kind in ((37, 41, "random"), (side, side, "random"), (side, side + 6, "extreme"), (29 + crop, 51, "extreme"), (40, 33, "near")):
        if kind == "random":
            a, b = rng.integers(0, 256, (H, W, Cc), dtype=np.uint8), rng.integers(0, 256, (H, W, Cc), dtype=np.uint8)
        elif kind == "extreme":                                     # a = 0, b = 255: S1 = -255 n (high word all ones), S2 = 65025 n
            a, b = np.zeros((H, W, Cc), np.uint8), np.full((H, W, Cc), 255, np.uint8)
        else:                                                       # a super-resolved image and its target: small differences of both signs
            a = rng.integers(0, 256, (H, W, Cc), dtype=np.uint8)
            b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, (H, W, Cc)), 0, 255).astype(np.uint8)
        want = _shift_reference(a, b, crop, m)
        if kind == "extreme":
            n = (H - 2 * crop - m) * (W - 2 * crop - m)
            assert (want[0::2] == -255 * n).all() and (want[1::2] == 65025 * n).all()
        got = _shift_run(a, b, crop, m)
        assert got.dtype == np.int64 and np.array_equal(got, want), (H, W, kind, int((got != want).sum()))


@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_shift_sums_past_the_row_block_cap(kind):
    """3 x 174763 = 256 * 2048 + 1 pixels: the first window at which a thread of the 256 row blocks runs a ninth trip"""
    H, W, Cc = 3, 174763, 3
    assert H * W == past_cap(SHIFT_PER_BLOCK, SHIFT_CAP)
    rng = np.random.default_rng(5)
    if kind == "random":
        a, b = rng.integers(0, 256, (H, W, Cc), dtype=np.uint8), rng.integers(0, 256, (H, W, Cc), dtype=np.uint8)
    else:
        a, b = np.zeros((H, W, Cc), np.uint8), np.full((H, W, Cc), 255, np.uint8)
    assert np.array_equal(_shift_run(a, b, 0, 0), _shift_reference(a, b, 0, 0))


def test_shift_sums_where_a_wave_partial_passes_2_to_31():
    """a = 0, b = 255 over 8192 x 8800 pixels: the 256 x 256 threads of the capped grid sum 1100 pixels each, so a lane holds 1100 * 65025 and
    the last level of the wave reduction carries 32 of those, 2.29e9 - a POSITIVE 64-bit value whose low word has its top bit set, which the
    shuffle of two 32-bit halves must not sign-extend into the high word.  (The negative sums of the smaller cases cannot show that: a
    sign-extended negative low word reproduces their all-ones high word.)"""
    H, W = 8192, 8800
    per_thread = H * W // (SHIFT_CAP * 256)
    assert per_thread * SHIFT_CAP * 256 == H * W and 2 ** 31 <= 32 * per_thread * 65025 < 2 ** 32
    a, b = np.zeros((H, W, 1), np.uint8), np.full((H, W, 1), 255, np.uint8)
    want = _shift_reference(a, b, 0, 0)
    assert want.tolist() == [-255 * H * W, 65025 * H * W]
    assert np.array_equal(_shift_run(a, b, 0, 0), want)


def test_shift_sums_return_codes():
    hip, L = _hip()
    ga, da = _bytes_from(np.zeros((40, 40, 4), np.uint8))
    go, out = _words(17 * 17 * 8, torch.int64)
    st = hip.stream_ptr()

    def call(H, W, Cc, crop, m):
        return L.ssr_metric_shift_sums(da.data_ptr(), da.data_ptr(), H, W, Cc, crop, m, out.data_ptr(), st)
    assert call(40, 40, 3, 0, 16) == EINVAL and call(30, 30, 5, 0, 0) == EINVAL
    assert call(16, 40, 3, 4, 8) == EINVAL and call(40, 8, 3, 0, 8) == EINVAL and call(8, 8, 1, 4, 0) == EINVAL       # empty windows
    torch.cuda.synchronize()
    assert bool((ibits(go.t) == go.sent).all()) and go.margins_intact()                                              # not even the memset ran


# ================================================================================================ ssr_metric_ssim_sums
def _ssim_map(a, b):
    """the SSIM map of one channel from the pieces of oracle/metrics_oracle.py (_ssim without its final mean)"""
    from oracle import metrics_oracle as M
    a, b = a.astype(np.float64), b.astype(np.float64)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    g = M._gauss()
    window = np.outer(g, g)
    mu1, mu2 = M._filter_valid(a, window), M._filter_valid(b, window)
    s1 = M._filter_valid(a ** 2, window) - mu1 ** 2
    s2 = M._filter_valid(b ** 2, window) - mu2 ** 2
    s12 = M._filter_valid(a * b, window) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 ** 2 + mu2 ** 2 + c1) * (s1 + s2 + c2))
    assert smap.mean() == M._ssim(a, b)                            # the oracle's own map
    return smap


def _ssim_bound(smap):
    """|device sum - fsum(map)| in units of fp64 roundings.
    One window sum (m, s11, ...): the kernel adds 11 + 11 products (<= 24 roundings on the longest chain), the oracle 121 (<= 122); both
    are sums of non-negative terms of total size <= 255^2, so each is within 24 U64 resp. 122 U64 of the exact value relatively; the
    squares m1^2 double the relative error of m1 and add one rounding.  Hence for v = s11 - m1^2 (and s22 - m2^2, s12 - m1 m2), whose
    two terms are up to 255^2 each while the difference may be 0:   dv <= (146 + 2 * 146 + 2 + 2) U64 * 255^2 = 442 U64 * 255^2.
    With SSIM = A B / (D E), A = 2 m1 m2 + C1 <= D = m1^2 + m2^2 + C1 (all terms positive: relative errors <= 2 * 146 + 4 each), B = 2 cov + C2
    (absolute error 2 dv, B may be near 0) and E = v1 + v2 + C2 >= C2 (absolute error 2 dv), |SSIM| <= 1:
        per pixel   (2 * 296 + 4) U64 + 2 dv / C2 + 2 dv / C2      (A, D and the three operations; B; E)
    The block sum: ceil(n / (grid * 256)) serial adds per thread, 8 tree levels, then one atomic add per block in arrival order - each
    rounds a partial sum of at most sum |map|."""
    n = smap.size
    grid = max(1, min((n + SSIM_PER_BLOCK - 1) // SSIM_PER_BLOCK, SSIM_CAP))
    c2 = (0.03 * 255) ** 2
    dv = 442 * U64 * 255.0 ** 2
    per_pixel = 596 * U64 + 4 * dv / c2
    depth = -(-n // (grid * 256)) + 8 + grid
    return n * per_pixel + depth * U64 * float(np.abs(smap).sum())


def _ssim_images(kind, H, W, Cc, seed):
    rng = np.random.default_rng(seed)
    if kind == "const_same":
        a = np.full((H, W, Cc), 200, np.uint8)
        return a, a.copy()
    if kind == "const_diff":
        return np.full((H, W, Cc), 255, np.uint8), np.full((H, W, Cc), 3, np.uint8)
    a = rng.integers(0, 256, (H, W, Cc), dtype=np.uint8)
    if kind == "random":
        return a, rng.integers(0, 256, (H, W, Cc), dtype=np.uint8)
    return a, np.clip(a.astype(np.int64) + rng.integers(-9, 10, (H, W, Cc)), 0, 255).astype(np.uint8)       # "near"


def _ssim_check(tag, kind, H, W, Cc, crop):
    hip, L = _hip()
    a, b = _ssim_images(kind, H, W, Cc, H * W + Cc)
    ga, da = _bytes_from(a)
    gb, db = _bytes_from(b)
    a0, b0 = ga.buf.clone(), gb.buf.clone()
    go, out = _words(Cc, torch.float64)
    out.fill_(123.0)                                               # overwritten, not added to
    hip.check(L.ssr_metric_ssim_sums(da.data_ptr(), db.data_ptr(), H, W, Cc, crop, out.data_ptr(), hip.stream_ptr()), "ssim_sums")
    got = out.cpu().numpy()
    sl = slice(crop, H - crop)
    worst = 0.0
    for c in range(Cc):
        smap = _ssim_map(a[sl, crop:W - crop, c], b[sl, crop:W - crop, c])
        assert smap.shape == (H - 2 * crop - 10, W - 2 * crop - 10)
        want, bound = math.fsum(smap.reshape(-1)), _ssim_bound(smap)
        assert bound <= 1e-9 * smap.size                           # no looser than rel = 1e-9 on a mean of order 1
        if kind in ("const_same", "near"):
            assert bound <= 1e-9 * abs(want)
        err = abs(float(got[c]) - want)
        worst = max(worst, err / bound)
        assert err <= bound, (tag, kind, c, err, bound)
    note("ssim_sums", f"{tag} {kind} {H}x{W}x{Cc} crop {crop}: max |sum - fsum(f64 map)| / bound", worst, 1.0)
    assert go.margins_intact() and torch.equal(ibits(ga.buf), ibits(a0)) and torch.equal(ibits(gb.buf), ibits(b0))


@pytest.mark.parametrize("kind", ["const_same", "const_diff", "random", "near"])
@pytest.mark.parametrize("H,W,Cc,crop", [(11, 11, 1, 0), (11, 11, 3, 0), (12, 27, 3, 0), (12, 27, 1, 0), (19, 19, 3, 4), (31, 45, 3, 4), (40, 37, 1, 4)])
def test_ssim_sums_per_channel(H, W, Cc, crop, kind):
    _ssim_check("small", kind, H, W, Cc, crop)


@pytest.mark.parametrize("kind", ["near", "random"])
def test_ssim_sums_past_the_block_cap(kind):
    """5 x 52429 = 1024 * 256 + 1 outputs: the first window at which a thread of the 1024 blocks runs a second trip"""
    H, W = 15, 52439
    assert (H - 10) * (W - 10) == past_cap(SSIM_PER_BLOCK, SSIM_CAP)
    _ssim_check("past_cap", kind, H, W, 1, 0)


def test_ssim_sums_return_codes():
    hip, L = _hip()
    ga, da = _bytes_from(np.zeros((20, 20, 3), np.uint8))
    go, out = _words(3, torch.float64)
    st = hip.stream_ptr()
    for H, W, crop in ((10, 20, 0), (20, 10, 0), (18, 20, 4), (20, 17, 4)):                 # H - 2 crop - 10 <= 0: no window
        assert L.ssr_metric_ssim_sums(da.data_ptr(), da.data_ptr(), H, W, 3, crop, out.data_ptr(), st) == EINVAL
    assert L.ssr_metric_ssim_sums(da.data_ptr(), da.data_ptr(), 20, 20, 0, 0, out.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((ibits(go.t) == go.sent).all()) and go.margins_intact()


def test_ssim_sums_on_a_second_device_of_the_same_process():
    """the Gaussian window is a __constant__ symbol, one copy per device: after a call on device 0 a call with device 1 current must
    upload it there too (a window of zeros gives SSIM = 1 for every pixel and no error)"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices: the per-device upload of the SSIM window cannot be told apart on one")
    for dev in (0, 1):
        with torch.cuda.device(dev):
            _ssim_check(f"device {dev}", "random", 12, 27, 3, 0)
            _ssim_check(f"device {dev}", "near", 31, 45, 3, 4)


# ================================================================================================ ssr_usm_sharp
USM_BAND = 0.02                # no pixel's |residual| * 255 may lie this close to the threshold 10: a condition on the INPUT, not a tolerance
# relative error of one fp32 Gaussian weight gk = __expf(-d^2 / 128): the argument is exact (d^2 <= 625, a division by 2^7); the HIP
# documentation gives the intrinsic 1 ulp (2 U relative); it is evaluated as exp2(x * log2(e)), and the rounding of that product at
# |x| <= 625 / 128 moves the result by another |x| log2(e) ln(2) * 2 U <= 9.8 U
USM_EW = (2 + 9.8) * U
# one separable pass over values in [0, 1]: 51 products and 51 sums on the longest chain (52 U), the sum of the weights (51 U), its
# reciprocal and the final product (2 U), and the weight errors in numerator and denominator (2 EW)
USM_PASS = (52 + 51 + 2) * U + 2 * USM_EW


def _usm_bounds(in_scale_exact):
    """first-order bounds, all values in [0, 1] (|residual| <= 1, |sharp - v| <= 1 / 2):
    dv     the scaled input fl(u8 * fl(1 / 255)) against u8 / 255: 2 U (0 where in_scale = 1)
    blur   two passes, the input error carried through (weights sum to 1), and the oracle's own 2-D kernel rounded to fp32 (U)
    res    v - blur: both errors and one rounding
    sharp  clip(v + 0.5 res): dv, half the residual's error, a product and a sum of values <= 1.5 (3 U)
    soft   two passes over the exact 0 / 1 mask (exact by the guard band) and the oracle's kernel rounding
    out    soft sharp + (1 - soft) v: soft's error times |sharp - v| <= 1 / 2, sharp's and v's errors (soft, 1 - soft <= 1), 4 roundings"""
    dv = 0.0 if in_scale_exact else 2 * U
    blur = 2 * USM_PASS + dv + U
    res = blur + dv + U
    sharp = dv + 0.5 * res + 3 * U
    soft = 2 * USM_PASS + U
    return res, 0.5 * soft + sharp + dv + 4 * U


def _usm_residual255(img64):
    from oracle import esrgan_oracle as O
    k1 = O.usm_gaussian_kernel1d(50, 0.0)
    k2 = torch.outer(k1, k1).to(torch.float32)                     # as usm_sharp builds it
    return (img64 - O.filter2d(img64, k2)).abs() * 255


@functools.lru_cache(maxsize=None)
def _usm_image(B, H, W):
    """the uint8-valued image of the earlier test, with every pixel whose |residual| * 255 lies within USM_BAND of the threshold moved
    by three grey levels towards mid-range, until none is left: (image, its |residual| * 255 in float64)"""
    torch.manual_seed(B + H)
    base = torch.rand(B, 3, H // 4 + 1, W // 4 + 1)
    img = torch.nn.functional.interpolate(base, size=(H, W), mode="bilinear") + 0.08 * torch.randn(B, 3, H, W)
    u8 = (img.clamp(0, 1) * 255).round()
    for _ in range(20):
        r255 = _usm_residual255(u8.double() / 255)
        near = (r255 - 10.0).abs() < USM_BAND
        if not bool(near.any()):
            return u8, r255
        u8 = torch.where(near, u8 + torch.where(u8 < 128, 3.0, -3.0), u8)
    raise AssertionError("the guard band did not clear")


# in_scale = 1 / 255 on uint8-valued input at every size; in_scale = 1 on [0, 1] input at the two smallest (the float64 oracle is a 2601-tap
# convolution: the largest case takes seconds as it is)
USM_CASES = [(1, 26, 26, True), (1, 26, 128, True), (1, 127, 129, True), (2, 128, 128, True), (1, 40, 52, True), (1, 26, 26, False), (1, 26, 128, False)]


@pytest.mark.parametrize("B,H,W,scaled", USM_CASES, ids=[f"{b * 3}x{h}x{w}-{'u8' if s else 'unit'}" for b, h, w, s in USM_CASES])
def test_usm_sharp_matches_oracle(B, H, W, scaled):
    """ssr_usm_sharp (separable 51-tap Gaussian in LDS, reflect padding) against the oracle's 2-D restatement of BasicSR's USMSharp in
    float64 (feed_data: ssr_esrgan_model.py:108-109), EVERY element to the derived bound.  The residual mask is a threshold: the inputs
    are built so that no pixel lies within USM_BAND of it, which is asserted on the reference alone before the kernel is looked at."""
    from oracle import esrgan_oracle as O
    hip, L = _hip()
    u8, r255 = _usm_image(B, H, W)
    x = u8 if scaled else (u8 / 255).float()                       # what the kernel reads
    img64 = u8.double() / 255 if scaled else x.double()            # what the reference operation is applied to
    if not scaled:
        r255 = _usm_residual255(img64)
    gap = float((r255 - 10.0).abs().min())
    masked = float((r255 > 10.0).double().mean())
    e_res, e_out = _usm_bounds(not scaled)
    assert gap >= USM_BAND and 0.02 < masked < 0.98                # the precondition, and both mask values occur
    # fp32 moves |residual| * 255 by at most e_res * 255 (4.0e-3: the summation error alone is 1.6e-3, the rest the weights of __expf and the
    # normalisation) and the product with 255 by one rounding more: the band is over four times that, so the device's mask IS the oracle's
    assert USM_BAND > 4 * (e_res * 255 + 2 * U * 10)
    assert e_out <= 2e-5                                           # no looser than the bound the 99.9 % were held to before
    ref = O.usm_sharp(img64)
    gs, gd = guarded_from(x), Guarded(x.numel())
    before = gs.buf.clone()
    hip.check(L.ssr_usm_sharp(gs.ptr(), gd.ptr(), B * 3, H, W, 1.0 / 255 if scaled else 1.0, 0.5, 10.0, hip.stream_ptr()), "ssr_usm_sharp")
    err, ratio = within(gd.t.cpu().view_as(ref), ref, e_out)
    note("usm_sharp_matches_oracle", f"{B * 3} planes {H}x{W} {'u8 / 255' if scaled else '[0, 1]'} (gap {gap:.3f}, {masked:.0%} masked): max |out - f64|", err, e_out)
    assert ratio <= 1.0
    assert gd.margins_intact() and torch.equal(ibits(gs.buf), ibits(before))


def test_usm_sharp_return_codes():
    hip, L = _hip()
    gs, gd = guarded_from(torch.zeros(113 * 145)), Guarded(113 * 145)
    st = hip.stream_ptr()
    assert L.ssr_usm_sharp(gs.ptr(), gd.ptr(), 1, 25, 26, 1.0, 0.5, 10.0, st) == EINVAL
    assert L.ssr_usm_sharp(gs.ptr(), gd.ptr(), 1, 26, 25, 1.0, 0.5, 10.0, st) == EINVAL
    assert L.ssr_usm_sharp(gs.ptr(), gd.ptr(), 1, 113, 145, 1.0, 0.5, 10.0, st) == EUNSUP          # 16 385 pixels
    assert L.ssr_usm_sharp(gs.ptr(), gd.ptr(), 0, 26, 26, 1.0, 0.5, 10.0, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((ibits(gd.t) == gd.sent).all()) and gd.margins_intact()
