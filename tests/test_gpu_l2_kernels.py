"""GPU: the kernels of csrc/l2net.hip (what lies between the convolutions of SRCNN and HighResNet), each called through the C ABI and
held to the host restatements of satlas_super_resolution_amd/l2_reference.py.

  * ssr_prelu_reflect_fwd and the data gradient of ssr_prelu_reflect_bwd are float32 restatements bit for bit: the forward is one
    multiply per element (and one exact doubling, one add); the backward's fold is ONE running float32 sum started with its first term,
    rows in increasing padded row index, columns in increasing padded column index inside a row, the first gradient buffer's terms
    before the second's.
  * d loss / d slope is a sum of n float32 products accumulated in float64 and rounded once: against the float64 sum it is held to the
    standard forward-error bound n * 2^-24 * sum|terms| (n roundings at most, each relative to a partial sum bounded by sum|terms|).
  * the tail (PixelShuffle, two 1 x 1 convolutions, two PReLUs) is float32 sums in channel order: an output is a chain of at most
    K = Cm + Co + 4 roundings per stage, held to K * 2^-24 * (sum of the magnitudes of the terms that enter it), computed in float64.
  * every output buffer lies between NaN-sentinel margins that must come back bit-unchanged; so must the channels of a wider
    buffer outside the written slice.
U = 2^-24 is the unit roundoff of float32."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EINVAL, EUNSUP = -1, -2
SENT = 0x7FC5A5A5
MARGIN = 64


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _ref():
    from satlas_super_resolution_amd import l2_reference
    return l2_reference


class Guarded:
    """a float32 device buffer of `shape` between two sentinel margins, itself filled with the sentinel"""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(np.prod(shape))
        self.buf = torch.empty(self.n + 2 * MARGIN, dtype=torch.float32, device="cuda")
        self.buf.view(torch.int32).fill_(SENT)
        self.t = self.buf[MARGIN:MARGIN + self.n].view(self.shape)

    def margins_intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:MARGIN] == SENT).all()) and bool((b[MARGIN + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf.view(torch.int32) == SENT).all())


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_case(rng, N, H, W, Cc, with_mask, with_res):
    R = _ref()
    pre = rng.standard_normal((N, H, W, Cc)).astype(np.float32)
    pre[0, 0, 0, 0] = 0.0                       # PReLU at exactly 0 counts as negative
    keep = rng.random((N, H, W, Cc)) < 0.5 if with_mask else None
    words = None
    if with_mask:
        words = R.pack_mask_nhwc(torch.from_numpy(keep).permute(0, 3, 1, 2))
    res = rng.standard_normal((N, H + 2, W + 2, Cc)).astype(np.float32) if with_res else None
    return pre, keep, words, res


SHAPES = [(2, 2), (3, 5), (8, 8), (6, 10)]
CHANNELS = [8, 32, 40]


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_prelu_reflect_forward_is_a_float32_restatement(hw, Cc):
    hip, lib = _hip()
    R = _ref()
    H, W = hw
    rng = np.random.default_rng(H * 100 + W * 10 + Cc)
    for with_mask, with_res, pad in ((False, False, 1), (True, False, 1), (True, True, 1), (True, True, 0)):
        pre, keep, words, res = make_case(rng, 2, H, W, Cc, with_mask, with_res)
        a = np.float32(0.173)
        out = Guarded((2, H + 2 * pad, W + 2 * pad, Cc))
        d = hip.PreluReflectDesc()
        d.N, d.H, d.W, d.C = 2, H, W, Cc
        pre_d, slope_d = dev(pre), dev(np.array([a], dtype=np.float32))
        d.pre, d.slope = hip.view(pre_d), slope_d.data_ptr()
        words_d = dev(words.view(np.int32)) if with_mask else None
        d.mask = words_d.data_ptr() if with_mask else None
        d.group = d.fold = 1
        d.out, d.out_pad = hip.View(out.t.data_ptr(), Cc, 0), pad
        res_d = dev(res) if with_res else None
        if with_res:
            d.res, d.res_pad = hip.view(res_d), 1
        assert lib.ssr_prelu_reflect_fwd(C.byref(d), None) == 0
        torch.cuda.synchronize()
        want = R.prelu_reflect_fwd_np(pre, a, keep, res[:, 1:-1, 1:-1] if with_res else None, pad)
        assert torch.equal(bits(out.t), bits(torch.from_numpy(want))), (hw, Cc, with_mask, with_res, pad)
        assert out.margins_intact()


def test_prelu_reflect_writes_a_channel_slice_of_another_image_and_nothing_else():
    """group 3, fold 2 (HighResNet with 3 revisits): image b*3 + r -> image b*2 + r % 2, channel half r // 2 of a buffer twice as wide
    (cs > C, coff > 0); the slot of the absent fourth revisit, the channels in front of the slice and the margins stay untouched"""
    hip, lib = _hip()
    R = _ref()
    B, G, Fd, H, W, Cc, coff = 2, 3, 2, 3, 5, 8, 8
    cs = coff + 2 * Cc
    rng = np.random.default_rng(5)
    pre, keep, words, _ = make_case(rng, B * G, H, W, Cc, True, False)
    a = np.float32(0.3)
    out = Guarded((B * Fd, H + 2, W + 2, cs))
    d = hip.PreluReflectDesc()
    d.N, d.H, d.W, d.C = B * G, H, W, Cc
    pre_d, slope_d, words_d = dev(pre), dev(np.array([a], dtype=np.float32)), dev(words.view(np.int32))
    d.pre, d.slope, d.mask = hip.view(pre_d), slope_d.data_ptr(), words_d.data_ptr()
    d.group, d.fold = G, Fd
    d.out, d.out_pad = hip.View(out.t.data_ptr(), cs, coff), 1
    assert lib.ssr_prelu_reflect_fwd(C.byref(d), None) == 0
    torch.cuda.synchronize()
    want = R.prelu_reflect_fwd_np(pre, a, keep, None, 1)
    got = out.t.cpu()
    gb = bits(out.t)
    written = torch.zeros(gb.shape, dtype=torch.bool)
    for b in range(B):
        for r in range(G):
            img, sl = b * Fd + r % Fd, coff + (r // Fd) * Cc
            assert torch.equal(bits(got[img, :, :, sl:sl + Cc]), bits(torch.from_numpy(want[b * G + r])))
            written[img, :, :, sl:sl + Cc] = True
    assert bool((gb[~written] == SENT).all()), "something outside the slices was written"
    assert out.margins_intact()


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("Cc", CHANNELS)
def test_prelu_reflect_backward_data_gradient_bit_exact_slope_gradient_bounded(hw, Cc):
    hip, lib = _hip()
    R = _ref()
    H, W = hw
    rng = np.random.default_rng(7 * H + W + Cc)
    N = 2
    for with_mask, g_pad, with_g2, g2_pad in ((False, 1, False, 1), (True, 1, True, 1), (True, 1, True, 0), (True, 0, False, 1)):
        pre, keep, words, _ = make_case(rng, N, H, W, Cc, with_mask, False)
        a = np.float32(0.21)
        g = rng.standard_normal((N, H + 2 * g_pad, W + 2 * g_pad, Cc)).astype(np.float32)
        g2 = rng.standard_normal((N, H + 2 * g2_pad, W + 2 * g2_pad, Cc)).astype(np.float32) if with_g2 else None
        dpre = Guarded((N, H, W, Cc))
        tsum = Guarded((N, H, W, Cc))
        pre_d, slope_d, g_d = dev(pre), dev(np.array([a], dtype=np.float32)), dev(g)
        words_d = dev(words.view(np.int32)) if with_mask else None
        g2_d = dev(g2) if with_g2 else None
        dslope = torch.full((1,), 0.5, device="cuda")
        partial = torch.zeros(hip.L2_SLOTS, dtype=torch.float64, device="cuda")
        d = hip.PreluReflectDesc()
        d.N, d.H, d.W, d.C = N, H, W, Cc
        d.pre, d.slope = hip.view(pre_d), slope_d.data_ptr()
        d.mask = words_d.data_ptr() if with_mask else None
        d.group = d.fold = 1
        d.g, d.g_pad = hip.view(g_d), g_pad
        if with_g2:
            d.g2, d.g2_pad = hip.view(g2_d), g2_pad
        d.dpre = hip.View(dpre.t.data_ptr(), Cc, 0)
        d.tsum = hip.View(tsum.t.data_ptr(), Cc, 0)
        d.dslope, d.partial = dslope.data_ptr(), partial.data_ptr()
        assert lib.ssr_prelu_reflect_bwd(C.byref(d), None) == 0
        torch.cuda.synchronize()
        first = float(dslope.item())
        want, terms = R.prelu_reflect_bwd_np(pre, a, g, g_pad, keep, g2, g2_pad)
        assert torch.equal(bits(dpre.t), bits(torch.from_numpy(want))), (hw, Cc, with_mask, g_pad, with_g2, g2_pad)
        t_want = R.fold_np(g, H, W, g_pad)
        if with_g2:
            t_want = R.fold_np(g2, H, W, g2_pad, acc=t_want)
        assert torch.equal(bits(tsum.t), bits(torch.from_numpy(t_want)))
        assert dpre.margins_intact() and tsum.margins_intact()
        # slope gradient: 0.5 (what was there) + the sum; n products, fp64 accumulation, one rounding to fp32, one fp32 add
        n = terms.size
        exact = float(terms.sum())
        bound = n * U * float(np.abs(terms).sum()) + 2 * U * (abs(exact) + 0.5)
        print(f"prelu_reflect_bwd {hw} C={Cc}: slope-gradient error {abs(first - 0.5 - exact):.3e}, bound {bound:.3e}")
        assert abs(first - 0.5 - exact) <= bound
        # a second launch gives the same bytes
        dslope.fill_(0.5)
        assert lib.ssr_prelu_reflect_bwd(C.byref(d), None) == 0
        torch.cuda.synchronize()
        assert float(dslope.item()) == first
        assert torch.equal(bits(dpre.t), bits(torch.from_numpy(want)))


def test_prelu_reflect_backward_reads_the_mapped_slices():
    hip, lib = _hip()
    R = _ref()
    B, G, Fd, H, W, Cc = 2, 4, 1, 6, 10, 8       # SRCNN: revisits as channels
    rng = np.random.default_rng(11)
    pre, keep, words, _ = make_case(rng, B * G, H, W, Cc, True, False)
    a = np.float32(0.4)
    g = rng.standard_normal((B, H + 2, W + 2, G * Cc)).astype(np.float32)
    pre_d, slope_d, words_d, g_d = dev(pre), dev(np.array([a], dtype=np.float32)), dev(words.view(np.int32)), dev(g)
    dpre = Guarded((B * G, H, W, Cc))
    dslope = torch.zeros(1, device="cuda")
    partial = torch.zeros(hip.L2_SLOTS, dtype=torch.float64, device="cuda")
    d = hip.PreluReflectDesc()
    d.N, d.H, d.W, d.C = B * G, H, W, Cc
    d.pre, d.slope, d.mask = hip.view(pre_d), slope_d.data_ptr(), words_d.data_ptr()
    d.group, d.fold = G, Fd
    d.g, d.g_pad = hip.view(g_d), 1
    d.dpre, d.dslope, d.partial = hip.View(dpre.t.data_ptr(), Cc, 0), dslope.data_ptr(), partial.data_ptr()
    assert lib.ssr_prelu_reflect_bwd(C.byref(d), None) == 0
    torch.cuda.synchronize()
    g_unmapped = np.stack([g[n // G, :, :, (n % G) * Cc:(n % G + 1) * Cc] for n in range(B * G)])
    want, _ = R.prelu_reflect_bwd_np(pre, a, g_unmapped, 1, keep)
    assert torch.equal(bits(dpre.t), bits(torch.from_numpy(want)))
    assert dpre.margins_intact()


def test_prelu_reflect_invalid_descriptors_launch_nothing():
    hip, lib = _hip()
    H, W, Cc, N = 3, 5, 8, 2
    pre = torch.randn(N, H, W, Cc, device="cuda")
    slope = torch.full((1,), 0.25, device="cuda")
    g = torch.randn(N, H + 2, W + 2, Cc, device="cuda")
    partial = torch.zeros(hip.L2_SLOTS, dtype=torch.float64, device="cuda")

    def fwd_desc(out):
        d = hip.PreluReflectDesc()
        d.N, d.H, d.W, d.C = N, H, W, Cc
        d.pre, d.slope, d.group, d.fold = hip.view(pre), slope.data_ptr(), 1, 1
        d.out, d.out_pad = hip.View(out.t.data_ptr(), Cc, 0), 1
        return d

    def bwd_desc(out, ds):
        d = hip.PreluReflectDesc()
        d.N, d.H, d.W, d.C = N, H, W, Cc
        d.pre, d.slope, d.group, d.fold = hip.view(pre), slope.data_ptr(), 1, 1
        d.g, d.g_pad = hip.view(g), 1
        d.dpre, d.dslope, d.partial = hip.View(out.t.data_ptr(), Cc, 0), ds.data_ptr(), partial.data_ptr()
        return d

    def breakers(is_fwd):
        yield "null pre", lambda d: setattr(d, "pre", hip.NULL_VIEW)
        yield "null slope", lambda d: setattr(d, "slope", None)
        yield "H < 2", lambda d: setattr(d, "H", 1)
        yield "W < 2", lambda d: setattr(d, "W", 1)
        yield "N <= 0", lambda d: setattr(d, "N", 0)
        yield "C % 4", lambda d: setattr(d, "C", 6)
        yield "pre narrower than coff + C", lambda d: setattr(d, "pre", hip.View(pre.data_ptr(), Cc, 4))
        yield "group < 1", lambda d: setattr(d, "group", 0)
        yield "N % group", lambda d: setattr(d, "group", 3)
        if is_fwd:
            yield "null out", lambda d: setattr(d, "out", hip.NULL_VIEW)
            yield "out narrower than its slices", lambda d: (setattr(d, "group", 2), setattr(d, "fold", 1))
            yield "out pad flag", lambda d: setattr(d, "out_pad", 2)
            yield "res narrower", lambda d: setattr(d, "res", hip.View(g.data_ptr(), Cc, 4))
        else:
            yield "null g", lambda d: setattr(d, "g", hip.NULL_VIEW)
            yield "g narrower", lambda d: setattr(d, "g", hip.View(g.data_ptr(), Cc, 4))
            yield "g2 narrower", lambda d: setattr(d, "g2", hip.View(g.data_ptr(), Cc, 4))
            yield "null dpre", lambda d: setattr(d, "dpre", hip.NULL_VIEW)
            yield "null dslope", lambda d: setattr(d, "dslope", None)
            yield "null partial", lambda d: setattr(d, "partial", None)

    assert lib.ssr_prelu_reflect_fwd(None, None) == EINVAL and lib.ssr_prelu_reflect_bwd(None, None) == EINVAL
    for what, brk in breakers(True):
        out = Guarded((N, H + 2, W + 2, Cc))
        d = fwd_desc(out)
        brk(d)
        assert lib.ssr_prelu_reflect_fwd(C.byref(d), None) == EINVAL, what
        torch.cuda.synchronize()
        assert out.untouched(), what
    for what, brk in breakers(False):
        out = Guarded((N, H, W, Cc))
        ds = torch.full((1,), 3.0, device="cuda")
        d = bwd_desc(out, ds)
        brk(d)
        assert lib.ssr_prelu_reflect_bwd(C.byref(d), None) == EINVAL, what
        torch.cuda.synchronize()
        assert out.untouched() and float(ds.item()) == 3.0, what


# ------------------------------------------------------------------------------------------------ the PixelShuffle tail
def _tail_setup(hidden, H, W, seed):
    hip, lib = _hip()
    z, Co, N = 4, 3, 2
    Cm = hidden // (z * z)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, H, W, hidden, generator=g)
    p = dict(w1=torch.randn(Cm, Cm, generator=g) * 0.7, b1=torch.randn(Cm, generator=g) * 0.3, s1=torch.tensor([0.2]),
             w2=torch.randn(Co, Cm, generator=g) * 0.7, b2=torch.randn(Co, generator=g) * 0.3, s2=torch.tensor([0.35]))
    return hip, lib, z, Co, N, Cm, x, p


def _tail_desc(hip, N, H, W, hidden, z, Co, x_d, p_d):
    d = hip.SrTailDesc()
    d.N, d.H, d.W, d.hidden, d.zoom, d.Cout = N, H, W, hidden, z, Co
    d.x = hip.view(x_d)
    for k in ("w1", "b1", "s1", "w2", "b2", "s2"):
        setattr(d, k, p_d[k].data_ptr())
    return d


@pytest.mark.parametrize("hidden", [16, 32, 128])
@pytest.mark.parametrize("hw", [(2, 2), (3, 5)])
def test_sr_tail_forward_and_backward(hidden, hw):
    R = _ref()
    H, W = hw
    hip, lib, z, Co, N, Cm, x, p = _tail_setup(hidden, H, W, hidden + H)
    x_d = x.cuda()
    p_d = {k: v.cuda() for k, v in p.items()}
    d = _tail_desc(hip, N, H, W, hidden, z, Co, x_d, p_d)
    y = Guarded((N, z * H, z * W, 8))
    d.y = hip.View(y.t.data_ptr(), 8, 0)
    assert lib.ssr_sr_tail_fwd(C.byref(d), None) == 0
    torch.cuda.synchronize()
    # float64 statement, with autograd for the gradients
    x64 = x.double().requires_grad_(True)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    y64 = R.sr_tail_reference(x64, p64["w1"], p64["b1"], p64["s1"], p64["w2"], p64["b2"], p64["s2"], z)
    # magnitudes: |b1| + |w1| |u|, then through the second layer (slopes <= 1 in magnitude)
    xa = R.sr_tail_reference(x.double().abs(), p["w1"].double().abs(), p["b1"].double().abs(), torch.tensor([1.0], dtype=torch.float64),
                             p["w2"].double().abs(), p["b2"].double().abs(), torch.tensor([1.0], dtype=torch.float64), z)
    K = Cm + Co + 4
    got = y.t.cpu()
    err = (got[..., :Co].double() - y64.detach()).abs()
    bound = 2 * K * U * xa
    print(f"sr_tail fwd hidden {hidden} {hw}: max error {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}")
    assert bool((err <= bound).all())
    assert bool((bits(got[..., Co:]) == SENT).all()) and y.margins_intact()
    # backward
    gy = torch.randn(N, z * H, z * W, 8)
    gy_d = gy.cuda()
    dx = Guarded((N, H, W, hidden))
    d.gy, d.dx = hip.view(gy_d), hip.View(dx.t.data_ptr(), hidden, 0)
    grads = {k: torch.full(v.shape, 0.25, device="cuda") for k, v in p.items()}
    for k in grads:
        setattr(d, "d" + k, grads[k].data_ptr())
    nbytes = lib.ssr_sr_tail_scratch_bytes(N, H, W, hidden, z, Co)
    assert nbytes > 0
    scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device="cuda")
    d.scratch = scratch.data_ptr()
    assert lib.ssr_sr_tail_bwd(C.byref(d), None) == 0
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in grads.items()}
    (y64 * gy[..., :Co].double()).sum().backward()
    # gradient magnitudes: the same chain with absolute values everywhere (every term of every sum enters with its magnitude)
    xm = x.double().abs().requires_grad_(True)
    pm = {k: v.double().abs().requires_grad_(True) for k, v in p.items()}
    one = torch.ones(1, dtype=torch.float64, requires_grad=True)
    ym = R.sr_tail_reference(xm, pm["w1"], pm["b1"], one, pm["w2"], pm["b2"], one, z)
    (ym * gy[..., :Co].double().abs()).sum().backward()
    e = (dx.t.cpu().double() - x64.grad).abs()
    b = 2 * K * U * xm.grad
    print(f"sr_tail bwd hidden {hidden} {hw}: dx max error {float(e.max()):.3e}")
    assert bool((e <= b + 1e-300).all()) and dx.margins_intact()
    npix = N * z * H * z * W
    # d / d slope = sum of g * min(0, pre): bounded by sum |g| |pre| with the magnitudes of the same chain
    with torch.no_grad():
        u = torch.nn.functional.pixel_shuffle(x.double().abs().permute(0, 3, 1, 2), z)
        p1m = torch.einsum("kc,nchw->nkhw", p["w1"].double().abs(), u) + p["b1"].double().abs()[None, :, None, None]
        p2m = torch.einsum("ok,nkhw->nohw", p["w2"].double().abs(), p1m) + p["b2"].double().abs()[None, :, None, None]
        gya = gy[..., :Co].double().abs().permute(0, 3, 1, 2)
        dam = torch.einsum("ok,nohw->nkhw", p["w2"].double().abs(), gya)
        slope_mag = {"s1": (p1m * dam).sum().reshape(1), "s2": (p2m * gya).sum().reshape(1)}
    for k in p:
        # per-pixel terms in fp32 (K roundings each), summed in fp64, one rounding, one fp32 add onto the 0.25 that was there
        mag = pm[k].grad if k not in ("s1", "s2") else slope_mag[k]
        ref = p64[k].grad
        got_k = first[k].cpu().double() - 0.25
        bound_k = (2 * K + npix) * U * mag + 2 * U * (ref.abs() + 0.25)
        ek = (got_k - ref).abs()
        print(f"  d{k}: max error {float(ek.max()):.3e}, smallest bound {float(bound_k.min()):.3e}")
        assert bool((ek <= bound_k).all()), k
    # the same bytes from a second launch
    for k in grads:
        grads[k].fill_(0.25)
    assert lib.ssr_sr_tail_bwd(C.byref(d), None) == 0
    torch.cuda.synchronize()
    for k in grads:
        assert torch.equal(bits(grads[k]), bits(first[k])), k


def test_sr_tail_invalid_descriptors_launch_nothing():
    H, W, hidden = 2, 2, 32
    hip, lib, z, Co, N, Cm, x, p = _tail_setup(hidden, H, W, 1)
    x_d = x.cuda()
    p_d = {k: v.cuda() for k, v in p.items()}
    assert lib.ssr_sr_tail_fwd(None, None) == EINVAL and lib.ssr_sr_tail_bwd(None, None) == EINVAL
    cases = [("null x", lambda d: setattr(d, "x", hip.NULL_VIEW), EINVAL), ("null w1", lambda d: setattr(d, "w1", None), EINVAL),
             ("hidden % zoom^2", lambda d: setattr(d, "hidden", 24), EINVAL), ("N <= 0", lambda d: setattr(d, "N", 0), EINVAL),
             ("x narrower", lambda d: setattr(d, "x", hip.View(x_d.data_ptr(), hidden, 8)), EINVAL),
             ("y narrower", lambda d: setattr(d, "y", hip.View(d.y.p, 8, 6)), EINVAL),
             ("Cout > 8", lambda d: setattr(d, "Cout", 9), EUNSUP)]
    for what, brk, code in cases:
        y = Guarded((N, z * H, z * W, 8))
        d = _tail_desc(hip, N, H, W, hidden, z, Co, x_d, p_d)
        d.y = hip.View(y.t.data_ptr(), 8, 0)
        brk(d)
        assert lib.ssr_sr_tail_fwd(C.byref(d), None) == code, what
        torch.cuda.synchronize()
        assert y.untouched(), what
    assert lib.ssr_sr_tail_scratch_bytes(N, H, W, 24, z, Co) == EINVAL


# ------------------------------------------------------------------------------------------------ dropout bits, loss
@pytest.mark.parametrize("n_words", [4, 1028, 4 * 70000])
def test_dropout_mask_bytes_equal_the_host_generator(n_words):
    hip, lib = _hip()
    R = _ref()
    seed, layer = 0x1234567890ABCDEF, 3
    step = torch.full((1,), 41, dtype=torch.int32, device="cuda")
    out = torch.empty(n_words + 2 * MARGIN, dtype=torch.int32, device="cuda")
    out.fill_(SENT)
    assert lib.ssr_dropout_mask(out[MARGIN:].data_ptr(), n_words, seed, step.data_ptr(), layer, 1, None) == 0
    torch.cuda.synchronize()
    want = R.philox_keep_bits(seed, 41, layer, n_words)
    assert np.array_equal(out[MARGIN:MARGIN + n_words].cpu().numpy().view(np.uint32), want)
    assert bool((out[:MARGIN] == SENT).all()) and bool((out[MARGIN + n_words:] == SENT).all())
    assert int(step.item()) == 42                                   # advance = 1
    assert lib.ssr_dropout_mask(out[MARGIN:].data_ptr(), n_words, seed, step.data_ptr(), layer, 0, None) == 0
    torch.cuda.synchronize()
    assert int(step.item()) == 42
    assert np.array_equal(out[MARGIN:MARGIN + n_words].cpu().numpy().view(np.uint32), R.philox_keep_bits(seed, 42, layer, n_words))
    for bad in ((None, 4), (out[MARGIN:].data_ptr(), 0), (out[MARGIN:].data_ptr(), 6)):
        assert lib.ssr_dropout_mask(bad[0], bad[1], seed, step.data_ptr(), layer, 0, None) == EINVAL
    assert lib.ssr_dropout_mask(out[MARGIN:].data_ptr(), 4, seed, None, layer, 0, None) == EINVAL


@pytest.mark.parametrize("npix", [1, 77, 24 * 40 * 2])
def test_mse_l1_loss_sums_and_combined_gradient(npix):
    hip, lib = _hip()
    Cc, cs = 3, 8
    g = torch.Generator().manual_seed(npix)
    a, b = torch.rand(npix, cs, generator=g), torch.rand(npix, cs, generator=g)
    a[0, 0] = b[0, 0]                                               # sign(0) = 0
    grad = Guarded((npix, cs))
    a_d, b_d = a.cuda(), b.cuda()
    sums = torch.full((2,), 0.125, device="cuda")
    partial = torch.zeros(2 * hip.L2_SLOTS, dtype=torch.float64, device="cuda")
    rc = lib.ssr_mse_l1_loss(hip.View(a_d.data_ptr(), cs, 0), hip.View(b_d.data_ptr(), cs, 0), hip.View(grad.t.data_ptr(), cs, 0), npix, Cc,
                             0.3, 0.4, sums.data_ptr(), partial.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    d32 = (a[:, :Cc] - b[:, :Cc])                                   # the kernel's one float32 subtraction
    d = d32.double()
    n = npix * Cc
    mse, mae = float((d * d).mean()), float(d.abs().mean())
    got = sums.cpu().double() - 0.125
    # n float32 -> float64 products summed in float64, one rounding, one float32 add onto 0.125
    assert abs(float(got[0]) - mse) <= 3 * U * (mse + 0.125) and abs(float(got[1]) - mae) <= 3 * U * (mae + 0.125)
    want = (0.3 * 2 / n) * d + (0.4 / n) * torch.sign(d)
    e = (grad.t.cpu()[:, :Cc].double() - want).abs()
    assert bool((e <= 4 * U * ((0.6 / n) * d.abs() + 0.4 / n)).all())            # two coefficient roundings, a product, a sum
    assert bool((bits(grad.t.cpu()[:, Cc:]) == SENT).all()) and grad.margins_intact()
    assert lib.ssr_mse_l1_loss(hip.NULL_VIEW, hip.View(b_d.data_ptr(), cs, 0), hip.NULL_VIEW, npix, Cc, 0.3, 0.4, sums.data_ptr(),
                               partial.data_ptr(), None) == EINVAL
    assert lib.ssr_mse_l1_loss(hip.View(a_d.data_ptr(), cs, 6), hip.View(b_d.data_ptr(), cs, 0), hip.NULL_VIEW, npix, Cc, 0.3, 0.4,
                               sums.data_ptr(), partial.data_ptr(), None) == EINVAL
