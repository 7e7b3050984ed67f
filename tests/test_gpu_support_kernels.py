"""GPU: the kernels around the convolutions - L1 and BCE-with-logits losses, the spectral-norm power iteration and its backward, the
fused Adam + EMA step - each called through the C ABI and held to a float64 restatement of the reference operation (torch's formulas,
not the kernel's code).  The bit-exact helpers and the weight packing are in tests/test_gpu_support_helpers.py.

Conventions of both modules:
  * U = 2^-24 is the unit roundoff of fp32 (round to nearest); a chain of k roundings is bounded by k U times the magnitude of the
    largest intermediate (first order, the "standard forward-error bound").  Every bound is written out next to its assertion.
  * where a result can be made exact (inputs that sum exactly, a gradient that is one product) the comparison is on integer bit patterns.
  * every output buffer lies between two margins filled with a NaN sentinel, and a strided view has the sentinel in the channels outside
    [coff, coff + C): all of them must come back bit-unchanged.
  * sizes: 1, sizes that are no multiple of 4 / 64 / 256, and the first size past the grid cap of the launch (csrc/misc.hip), where a
    thread runs one more trip of its grid-stride loop than the uncapped grid would give it.
Every test prints the largest error it saw next to the bound; with SSR_SUPPORT_KERNELS_REPORT=<file> the lines are appended to that file
(kept as profiles/support_kernels/observed_errors.txt)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                   # unit roundoff of fp32
MARGIN = 64                      # sentinel elements on each side of an output buffer (a multiple of 16 bytes in fp32 and bf16)
SENT = {4: 0x7FC5A5A5, 2: 0x7FC5}   # NaN bit patterns no kernel here produces
EINVAL, EUNSUP = -1, -2

# grid caps of csrc/misc.hip: (elements per block the host sizes the grid with, cap on the blocks)
L1_PER_BLOCK, LOSS_CAP_DEFAULT, LOSS_CAP_DET = 256 * 4, 1024, 256      # ssr_l1_loss / ssr_bce_logits_loss: grid_for(total, 256 * 4, det ? 256 : 1024)
SN_BWD_PER_BLOCK, SN_BWD_CAP = 256 * 8, 64                              # ssr_spectral_norm_bwd: grid_for(max_elems, 256 * 8, SSR_SN_BWD_SLOTS)
ADAM_PER_BLOCK, ADAM_CAP = 256 * 4, 2048                                # ssr_adam_step, ssr_axpby_f32: grid_for(n, 256 * 4, 2048)


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def grid_for(total, per_block, cap):
    """the host-side grid size of csrc/misc.hip"""
    return max(1, min((total + per_block - 1) // per_block, cap))


def past_cap(per_block, cap, multiple=1):
    """the smallest element count (a multiple of `multiple`) past per_block * cap: the first size at which the capped grid no longer
    covers `per_block` elements per block, so some thread runs one more trip than in any smaller launch"""
    n = per_block * cap + 1
    return (n + multiple - 1) // multiple * multiple


def ibits(t):
    """the bit patterns of a tensor as integers of the same width"""
    return t.detach().contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return torch.equal(ibits(a).cpu(), ibits(b).cpu())


class Guarded:
    """`n` elements of `dtype` on the device between two margins of sentinel elements; `shift` extra elements in front move the
    payload off 16-byte alignment.  The payload starts as sentinel too."""

    def __init__(self, n, dtype=torch.float32, shift=0):
        self.n, self.lo = n, MARGIN + shift
        self.buf = torch.empty(self.lo + n + MARGIN, dtype=dtype, device="cuda")
        self.sent = SENT[self.buf.element_size()]
        ibits(self.buf).fill_(self.sent)
        self.t = self.buf[self.lo:self.lo + n]

    def ptr(self):
        return self.t.data_ptr()

    def margins_intact(self):
        b = ibits(self.buf)
        return bool((b[:self.lo] == self.sent).all()) and bool((b[self.lo + self.n:] == self.sent).all())

    def channels_intact(self, cs, coff, nc):
        """payload seen as [npix, cs]: everything outside the columns [coff, coff + nc) is still the sentinel"""
        v = ibits(self.buf)[self.lo:self.lo + self.n].view(-1, cs)
        return bool((v[:, :coff] == self.sent).all()) and bool((v[:, coff + nc:] == self.sent).all())


def guarded_from(x, dtype=torch.float32, shift=0):
    g = Guarded(x.numel(), dtype, shift)
    g.t.copy_(x.reshape(-1).to(dtype))
    return g


def strided(data, cs, coff, dtype):
    """[npix, C] values (exact in `dtype`) as the channels [coff, coff + C) of a guarded [npix, cs] buffer: (Guarded, ssr_view)"""
    hip, _ = _hip()
    npix, nc = data.shape
    g = Guarded(npix * cs, dtype)
    v = g.t.view(npix, cs)
    v[:, coff:coff + nc] = data.to(dtype).cuda()
    return g, hip.view(v, coff)


def read_view(g, cs, coff, nc):
    return g.t.view(-1, cs)[:, coff:coff + nc].cpu()


_REPORT = []


def note(test, what, observed, bound):
    """one line per figure: what was measured on the device and the derived bound it was held to"""
    line = f"{test:<44} {what:<58} observed {observed:.3e}  bound {bound:.3e}"
    _REPORT.append(line)
    print(line)


@pytest.fixture(scope="module", autouse=True)
def _report_file(request):
    yield
    path = os.environ.get("SSR_SUPPORT_KERNELS_REPORT")
    if path and _REPORT:
        with open(path, "a") as f:
            f.write(f"# {request.module.__name__}\n" + "\n".join(_REPORT) + "\n")
        del _REPORT[:]


def within(got, ref, bound):
    """(largest error, largest error / bound) of |got - ref| <= bound, element by element, nothing left out"""
    err = (got.double() - ref.double()).abs()
    assert bool(torch.isfinite(got.double()).all())
    ratio = err / bound.clamp_min(1e-300) if torch.is_tensor(bound) else err / max(bound, 1e-300)
    return float(err.max()), float(ratio.max())


# ================================================================================================ 1. ssr_l1_loss
# channel strides / offsets (multiples of 8 as the header asks) of a, b and grad, all different
L1_LAYOUTS = {
    "dense": lambda nc: ((nc, 0), (nc, 0), (nc, 0)),
    "strided": lambda nc: ((16, 8), (24, 16), (24, 8)) if nc <= 8 else ((128, 64), (72, 8), (96, 32)),
}
# (npix, C): 1 element; 267 = 256 + 11 (one block, a second trip for 11 threads); 12 297 and 320 (no multiple of 4 / 64 / 256 resp. of
# 256); the first sizes past the deterministic cap (256 blocks x 1024) and the default cap (1024 x 1024) for C = 3 and C = 64; and the
# 1 200 003 elements whose block sums the exactness argument below was checked for
L1_SHAPES = [(1, 1), (89, 3), (4099, 3), (5, 64),
             (past_cap(L1_PER_BLOCK, LOSS_CAP_DET, 3) // 3, 3), (past_cap(L1_PER_BLOCK, LOSS_CAP_DEFAULT, 3) // 3, 3),
             (past_cap(L1_PER_BLOCK, LOSS_CAP_DEFAULT, 64) // 64, 64), (400001, 3)]


def _sixteenths(npix, nc, seed):
    """multiples of 1/16 in [-1.5, 1.5]: exact in bf16 (5 significant bits), a == b for 1 element in 49, and every sum of |a - b| over a
    block is a multiple of 1/16 below 2^24 / 16 - exact in fp32 in whatever order the block adds it"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-24, 25, (npix, nc), generator=g).double() / 16, torch.randint(-24, 25, (npix, nc), generator=g).double() / 16)


def _block_sums(absd, grid):
    """sum of |d| per block: element e of the flat [npix, C] order belongs to block (e // 256) % grid (256 threads, grid-stride)"""
    e = np.arange(absd.numel())
    return np.bincount((e // 256) % grid, weights=absd.reshape(-1).numpy(), minlength=grid)


def _l1_call(views, code, npix, nc, weight, loss_ptr):
    hip, L = _hip()
    return L.ssr_l1_loss(views[0], views[1], views[2], code, npix, nc, weight, loss_ptr, hip.stream_ptr())


def _l1_grad_bits(d, weight, dtype):
    """+-fl(fl(weight) * fl(1 / fl(total))), exactly 0 where a == b, rounded once more for bf16 storage"""
    wi = np.float32(weight) * (np.float32(1.0) / np.float32(d.numel()))
    return ibits((torch.sign(d).float() * float(wi)).to(dtype))


@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix,nc", L1_SHAPES, ids=[f"{p}x{c}" for p, c in L1_SHAPES])
def test_l1_loss_exact_inputs(npix, nc, dtype, layout):
    hip, L = _hip()
    code = hip.BF16 if dtype is torch.bfloat16 else hip.F32
    weight, total = 0.7, npix * nc
    a, b = _sixteenths(npix, nc, 11 * npix + nc)
    d = a - b
    absd = d.abs()
    lay = L1_LAYOUTS[layout](nc)
    ga, va = strided(a, *lay[0], dtype)
    gb, vb = strided(b, *lay[1], dtype)
    gg, vg = strided(torch.zeros(npix, nc, dtype=torch.float64), *lay[2], dtype)
    ibits(gg.t).fill_(gg.sent)
    a_before, b_before = ga.buf.clone(), gb.buf.clone()
    want_grad = _l1_grad_bits(d, weight, dtype)
    w32, invn = np.float32(weight), np.float32(1.0) / np.float32(total)

    # ---- deterministic mode: SSR_LOSS_SLOTS slots, block b the single writer of slot b
    G = grid_for(total, L1_PER_BLOCK, LOSS_CAP_DET)
    sums = _block_sums(absd, G)
    assert sums.max() * 16 < 2 ** 24                       # the exactness argument of _sixteenths holds for this case
    slots = Guarded(hip.LOSS_SLOTS)
    slots.t[:G] = 0.0                                      # slots G .. 255 keep the sentinel: they must stay untouched
    hip.check(_l1_call((va, vb, vg), code | hip.DETERMINISTIC, npix, nc, weight, slots.ptr()), "ssr_l1_loss")
    # fl(fl(s_b * weight) * invn): both products of exactly known operands, added to a zero slot - bit for bit
    want = torch.from_numpy(((sums.astype(np.float32) * w32) * invn).astype(np.float32))
    assert same_bits(slots.t[:G], want)
    assert bool((ibits(slots.t[G:]) == slots.sent).all()) and slots.margins_intact()
    assert torch.equal(ibits(read_view(gg, lay[2][0], lay[2][1], nc)), want_grad)     # every element written once, 0 where a == b
    assert gg.margins_intact() and gg.channels_intact(lay[2][0], lay[2][1], nc)
    # a second launch adds to the slots: slot + term, where the compiler may fuse the last product into the add - 1 ulp
    first = slots.t[:G].clone()
    hip.check(_l1_call((va, vb, hip.NULL_VIEW), code | hip.DETERMINISTIC, npix, nc, weight, slots.ptr()), "ssr_l1_loss")
    twice = (first.cpu().numpy() + want.numpy()).astype(np.float32)
    ulps = (ibits(slots.t[:G]).cpu().long() - ibits(torch.from_numpy(twice)).long()).abs().max()
    assert int(ulps) <= 1
    assert bool((ibits(slots.t[G:]) == slots.sent).all()) and slots.margins_intact()

    # ---- default mode: one atomic add per block into loss_out[0]
    G = grid_for(total, L1_PER_BLOCK, LOSS_CAP_DEFAULT)
    assert _block_sums(absd, G).max() * 16 < 2 ** 24
    loss64 = float(np.float64(w32) * float(absd.sum()) / total)
    for preload in (0.0, 0.75):
        ibits(gg.t).fill_(gg.sent)
        out = Guarded(1)
        out.t[0] = preload
        hip.check(_l1_call((va, vb, vg), code, npix, nc, weight, out.ptr()), "ssr_l1_loss")
        # the block sums are exact, so the error is two products per block term and G atomic adds, each rounding a partial sum that is
        # at most preload + loss (all terms >= 0): (G + 2) U (preload + loss)
        bound = (G + 2) * U * (preload + loss64)
        err = abs(float(out.t[0].double()) - (float(np.float32(preload)) + loss64))
        note("l1_loss_exact_inputs", f"{npix}x{nc} {dtype} {layout} preload {preload}: |loss - f64|", err, bound)
        assert err <= bound and out.margins_intact()
        assert torch.equal(ibits(read_view(gg, lay[2][0], lay[2][1], nc)), want_grad)
        assert gg.margins_intact() and gg.channels_intact(lay[2][0], lay[2][1], nc)
    assert torch.equal(ibits(ga.buf), ibits(a_before)) and torch.equal(ibits(gb.buf), ibits(b_before))     # inputs are only read


def _sum_depth(total, grid):
    """roundings on the longest chain of a block reduction of csrc/misc.hip: a thread adds ceil(total / (grid * 256)) terms serially,
    then 6 shuffle levels inside a wave and 2 levels over the 4 wave sums in LDS"""
    return -(-total // (grid * 256)) + 6 + 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "slots"])
def test_l1_loss_random_inputs(dtype, det):
    """random normal inputs (not exactly summable), strided views, past the cap of the mode"""
    hip, L = _hip()
    code = (hip.BF16 if dtype is torch.bfloat16 else hip.F32) | (hip.DETERMINISTIC if det else 0)
    nc, weight = 3, 1.0
    npix = past_cap(L1_PER_BLOCK, LOSS_CAP_DET if det else LOSS_CAP_DEFAULT, 3) // 3 + 1000
    total = npix * nc
    g = torch.Generator().manual_seed(5)
    a = torch.randn(npix, nc, generator=g).to(dtype).double()
    b = torch.randn(npix, nc, generator=g).to(dtype).double()
    b[::50] = a[::50]                                       # 2 % exact zeros of the difference
    d = a - b
    lay = L1_LAYOUTS["strided"](nc)
    ga, va = strided(a, *lay[0], dtype)
    gb, vb = strided(b, *lay[1], dtype)
    gg, vg = strided(torch.zeros(npix, nc, dtype=torch.float64), *lay[2], dtype)
    ibits(gg.t).fill_(gg.sent)
    G = grid_for(total, L1_PER_BLOCK, LOSS_CAP_DET if det else LOSS_CAP_DEFAULT)
    out = Guarded(hip.LOSS_SLOTS if det else 1)
    out.t[:G if det else 1] = 0.0
    hip.check(_l1_call((va, vb, vg), code, npix, nc, weight, out.ptr()), "ssr_l1_loss")
    # fl(a - b) has the sign of a - b and is 0 only where a == b: the gradient stays a bit-exact target
    assert torch.equal(ibits(read_view(gg, lay[2][0], lay[2][1], nc)), _l1_grad_bits(d, weight, dtype))
    assert gg.margins_intact() and gg.channels_intact(lay[2][0], lay[2][1], nc) and out.margins_intact()
    sums = _block_sums(d.abs(), G) * weight / total
    k = 1 + _sum_depth(total, G) + 2           # the subtraction, the block reduction, the two products
    if det:
        # per slot: k roundings of the block's own sum of |d| (all terms >= 0)
        err, ratio = within(out.t[:G].cpu(), torch.from_numpy(sums), torch.from_numpy(sums) * k * U)
        assert bool((ibits(out.t[G:]) == out.sent).all())
    else:
        # and G atomic adds on top, each at most at the size of the whole loss
        err, ratio = within(out.t[:1].cpu(), torch.tensor([sums.sum()]), float(sums.sum()) * (k + G) * U)
    note("l1_loss_random_inputs", f"{total} elements {dtype} {'slots' if det else 'atomic'}: max error / bound", ratio, 1.0)
    assert ratio <= 1.0


def test_l1_loss_optional_pointers_and_dtype_codes():
    hip, L = _hip()
    npix, nc, weight = 4099, 3, 0.25
    a, b = _sixteenths(npix, nc, 3)
    d = a - b
    ga, va = strided(a, 16, 8, torch.float32)
    gb, vb = strided(b, 24, 16, torch.float32)
    loss64 = weight * float(d.abs().sum()) / (npix * nc)
    G = grid_for(npix * nc, L1_PER_BLOCK, LOSS_CAP_DEFAULT)
    # every mode code that means fp32 storage: plain fp32, the split-bf16 code, and what storage_code() gives the mixed modes
    for code in sorted({hip.F32, hip.F32X3, hip.storage_code(hip.F32F), hip.storage_code(hip.F32H)}):
        gg, vg = strided(torch.zeros(npix, nc, dtype=torch.float64), 24, 8, torch.float32)
        ibits(gg.t).fill_(gg.sent)
        out = Guarded(1)
        out.t[0] = 0.0
        hip.check(_l1_call((va, vb, vg), code, npix, nc, weight, out.ptr()), "ssr_l1_loss")
        assert abs(float(out.t[0]) - loss64) <= (G + 2) * U * loss64                     # as in test_l1_loss_exact_inputs
        assert torch.equal(ibits(read_view(gg, 24, 8, nc)), _l1_grad_bits(d, weight, torch.float32))
        assert gg.margins_intact() and gg.channels_intact(24, 8, nc) and out.margins_intact()
    # grad = NULL_VIEW: the loss alone
    out = Guarded(1)
    out.t[0] = 0.0
    hip.check(_l1_call((va, vb, hip.NULL_VIEW), hip.F32, npix, nc, weight, out.ptr()), "ssr_l1_loss")
    assert abs(float(out.t[0]) - loss64) <= (G + 2) * U * loss64 and out.margins_intact()
    # loss_out = NULL: the gradient alone
    gg, vg = strided(torch.zeros(npix, nc, dtype=torch.float64), 24, 8, torch.float32)
    ibits(gg.t).fill_(gg.sent)
    hip.check(_l1_call((va, vb, vg), hip.F32, npix, nc, weight, None), "ssr_l1_loss")
    assert torch.equal(ibits(read_view(gg, 24, 8, nc)), _l1_grad_bits(d, weight, torch.float32))
    assert gg.margins_intact() and gg.channels_intact(24, 8, nc)
    # an unsupported storage code: SSR_EUNSUP and no launch (nothing written)
    ibits(gg.t).fill_(gg.sent)
    out = Guarded(1)
    for code in (hip.F32H3, 7, 7 | hip.DETERMINISTIC):
        assert _l1_call((va, vb, vg), code, npix, nc, weight, out.ptr()) == EUNSUP
    torch.cuda.synchronize()
    assert bool((ibits(gg.t) == gg.sent).all()) and bool((ibits(out.t) == out.sent).all())
    assert _l1_call((hip.NULL_VIEW, vb, vg), hip.F32, npix, nc, weight, out.ptr()) == EINVAL


# ================================================================================================ 2. ssr_bce_logits_loss
BCE_EDGES = [-100.0, 100.0, -88.8, 88.8, -20.0, 20.0, -17.0, 17.0, 0.0, 1e-8, -1e-8]
BCE_SIZES = [1, 267, 12297, past_cap(L1_PER_BLOCK, LOSS_CAP_DET), past_cap(L1_PER_BLOCK, LOSS_CAP_DEFAULT)]


def _logits(npix, dtype, seed):
    """random logits x 3 with the edge values in front (as many as fit), rounded to the storage type: what the kernel reads"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(npix, generator=g) * 3
    k = min(npix, len(BCE_EDGES))
    x[:k] = torch.tensor(BCE_EDGES[:k])
    return x.to(dtype).double()


def _bce_reference(x, target):
    """per-element BCE-with-logits, sigmoid and the logits, float64 (torch's own functions)"""
    t = torch.full_like(x, target)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction="none"), torch.sigmoid(x)


_BCE_CALLS = [(1.0, 1.0), (0.0, 1.0), (1.0, 0.1), (0.0, 0.1)]      # (target, weight) as train_step.py calls it
# the small sizes with every call on both views; the two sizes past the caps with the generator's and a discriminator's call on the
# padded view (8.4 M floats)
BCE_CASES = [(n, dt, t, w, padded) for n in BCE_SIZES[:3] for dt in (torch.float32, torch.bfloat16) for t, w in _BCE_CALLS
             for padded in (True, False)] + \
            [(n, dt, t, w, True) for n in BCE_SIZES[3:] for dt in (torch.float32, torch.bfloat16) for t, w in ((1.0, 0.1), (0.0, 1.0))]


@pytest.mark.parametrize("npix,dtype,target,weight,padded", BCE_CASES,
                         ids=[f"{n}-{'bf16' if dt is torch.bfloat16 else 'fp32'}-t{t:g}-w{w:g}-{'cs8' if p else 'dense'}"
                              for n, dt, t, w, p in BCE_CASES])
def test_bce_logits_loss(npix, dtype, target, weight, padded):
    hip, L = _hip()
    code = hip.BF16 if dtype is torch.bfloat16 else hip.F32
    cs = 8 if padded else 1                      # the discriminator plan stores its logits as channel 0 of an 8-channel buffer
    x = _logits(npix, dtype, npix)
    f, sig = _bce_reference(x, target)
    gx, vx = strided(x[:, None], cs, 0, dtype)
    w32, invn = np.float32(weight), np.float32(1.0) / np.float32(npix)
    wn = float(w32) / npix
    # ---- gradient, per element: weight * (sigmoid(x) - t) / npix.  The fp32 evaluation of this formula on the host is off by
    # 1.65 U weight / npix; 4 U leaves room for the device's expf and division (a figure from the host restatement, not the device).
    # bf16 storage rounds the fp32 result once more: half a bf16 ulp is at most 2^-8 (8 significant bits) of its magnitude.
    gref = (sig - target) * float(w32) / npix
    gbound = torch.full_like(gref, 4 * U * wn) + ((gref.abs() + 4 * U * wn) * 2.0 ** -8 if dtype is torch.bfloat16 else 0.0)
    # ---- loss and mean: the float64 sums, with the summation bound of the L1 loss (depth of the block reduction, two products, G
    # atomic adds) on the sum of magnitudes, plus 3 U max(|x|, 1) per element for max(x, 0) - x t + log1p(exp(-|x|)) evaluated in
    # fp32 (2.3 ulp in the host restatement)
    per_elem = 3 * U * x.abs().clamp_min(1.0)

    def check_grad(gg):
        got = read_view(gg, cs, 0, 1)[:, 0]
        err, ratio = within(got, gref, gbound)
        note("bce_logits_loss", f"{npix} {dtype} t={target} w={weight}: grad error / bound", ratio, 1.0)
        assert ratio <= 1.0
        assert gg.margins_intact() and gg.channels_intact(cs, 0, 1)
        # at +-100 the sigmoid saturates to exactly 0 / 1 in fp32: the gradient is the two products of exactly known operands
        for i, e in enumerate(BCE_EDGES[:min(2, npix)]):
            s = np.float32(1.0 if e > 0 else 0.0)
            want = torch.tensor([float((s - np.float32(target)) * w32 * invn)]).to(dtype)
            assert same_bits(got[i:i + 1].to(dtype), want), e

    for det in (False, True):
        G = grid_for(npix, L1_PER_BLOCK, LOSS_CAP_DET if det else LOSS_CAP_DEFAULT)
        k = _sum_depth(npix, G) + 2
        gg, vg = strided(torch.zeros(npix, 1, dtype=torch.float64), cs, 0, dtype)
        ibits(gg.t).fill_(gg.sent)
        n_out = hip.LOSS_SLOTS if det else 1
        lo, mo = Guarded(n_out), Guarded(n_out)
        for o in (lo, mo):
            o.t[:G if det else 1] = 0.0
        hip.check(L.ssr_bce_logits_loss(vx, vg, code | (hip.DETERMINISTIC if det else 0), npix, target, weight, lo.ptr(), mo.ptr(),
                                        hip.stream_ptr()), "ssr_bce_logits_loss")
        check_grad(gg)
        blk = (np.arange(npix) // 256) % G
        if det:
            refs = [np.bincount(blk, weights=v.numpy(), minlength=G) for v in (f, f.abs(), per_elem, x, x.abs())]
            sl, sl_abs, sl_pe, sm, sm_abs = [torch.from_numpy(r) for r in refs]
            _, r1 = within(lo.t[:G].cpu(), sl * wn, (k * U * sl_abs + sl_pe) * wn)
            _, r2 = within(mo.t[:G].cpu(), sm / npix, (k - 1) * U * sm_abs / npix)      # one product instead of two
            for o in (lo, mo):
                assert bool((ibits(o.t[G:]) == o.sent).all()) and o.margins_intact()
        else:
            _, r1 = within(lo.t.cpu(), (f.sum() * wn).reshape(1), float(((k + G) * U * f.abs().sum() + per_elem.sum()) * wn))
            _, r2 = within(mo.t.cpu(), (x.sum() / npix).reshape(1), float((k - 1 + G) * U * x.abs().sum() / npix))
            assert lo.margins_intact() and mo.margins_intact()
        note("bce_logits_loss", f"{npix} {dtype} t={target} w={weight} {'slots' if det else 'atomic'}: loss, mean error / bound", max(r1, r2), 1.0)
        assert r1 <= 1.0 and r2 <= 1.0
    # ---- the optional pointers: mean_out = NULL, then grad = NULL; loss_out accumulates over the two calls
    G = grid_for(npix, L1_PER_BLOCK, LOSS_CAP_DEFAULT)
    k = _sum_depth(npix, G) + 2
    gg, vg = strided(torch.zeros(npix, 1, dtype=torch.float64), cs, 0, dtype)
    ibits(gg.t).fill_(gg.sent)
    lo = Guarded(1)
    lo.t[0] = 0.0
    hip.check(L.ssr_bce_logits_loss(vx, vg, code, npix, target, weight, lo.ptr(), None, hip.stream_ptr()), "ssr_bce_logits_loss")
    check_grad(gg)
    ibits(gg.t).fill_(gg.sent)
    hip.check(L.ssr_bce_logits_loss(vx, hip.NULL_VIEW, code, npix, target, weight, lo.ptr(), None, hip.stream_ptr()), "ssr_bce_logits_loss")
    assert bool((ibits(gg.t) == gg.sent).all())
    # (the G atomic adds of the second call round partial sums of up to twice the loss: k + G and k + 2 G roundings)
    _, r = within(lo.t.cpu(), (2 * f.sum() * wn).reshape(1), float(((2 * k + 3 * G) * U * f.abs().sum() + 2 * per_elem.sum()) * wn))
    assert r <= 1.0 and lo.margins_intact()
    assert L.ssr_bce_logits_loss(vx, vg, 7, npix, target, weight, lo.ptr(), None, hip.stream_ptr()) == EUNSUP


# ================================================================================================ 3. ssr_spectral_norm
# (rows, cols, misalign): one table, so max_rows / max_cols exceed most items.  (5, 45): cols % 4 != 0.  (1, 48), (7, 576): the power
# iteration reads W^T u from tmp + rows, which is off 16 bytes - scalar by alignment; with power_iter = 0 they read v and take the
# vector path.  (64, 1152), (256, 4608) (the largest real layer: 18 KB per wave) and (64, 576): the vector path.  The last item is
# (64, 576) again with w one float into its parent: no row is 16-byte aligned - scalar by alignment at cols % 4 == 0.
SN_ITEMS = [(5, 45, 0), (1, 48, 0), (7, 576, 0), (64, 1152, 0), (256, 4608, 0), (64, 576, 0), (64, 576, 1)]
SN_EPS = 1e-12


def _sn_data(seed=0):
    """per item: W, u, v in float64 holding fp32 values; u, v normalised as torch initialises them; the twin shares its data"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for rows, cols, mis in SN_ITEMS:
        if mis:
            out.append(tuple(t.clone() for t in out[-1]))
            continue
        w = (torch.randn(rows, cols, generator=g) * 0.05).double()
        u = torch.nn.functional.normalize(torch.randn(rows, generator=g), dim=0, eps=SN_EPS).double()
        v = torch.nn.functional.normalize(torch.randn(cols, generator=g), dim=0, eps=SN_EPS).double()
        out.append((w, u, v))
    return out


def _sn_vector_path(rows, cols, mis, power_iter):
    """sn_wv_kernel's documented condition for 16-byte loads: cols % 4 == 0, 16-byte aligned rows and an aligned v source (tmp + rows
    under power iteration, v otherwise; the buffers of this test are 16-byte aligned)"""
    return cols % 4 == 0 and not mis and (rows % 4 == 0 if power_iter else True)


def _sn_reference(w, u, v, k_wv, power_iter):
    """torch.nn.utils.spectral_norm's step in float64 - v <- normalize(W^T u), u <- normalize(W v), sigma = u . (W v), eps 1e-12 - with
    first-order bounds of the fp32 evaluation.  gamma_k sum |W_ij| |x_j| bounds a dot product of chain length k; a normalisation adds
    2 ulp (square root and product; the sum of squares only has terms of one sign) and moves with the errors of its input."""
    rows, cols = w.shape
    aw = w.abs()
    if not power_iter:
        s = w @ v
        es = k_wv * U * (aw @ v.abs())
        k_fin = -(-rows // 256) + 6 + 2                              # sn_finish_kernel: one block of 256 threads over the rows
        sigma = u @ s
        e_sigma = u.abs() @ es + k_fin * U * (u.abs() @ s.abs())
        return u, v, sigma, None, None, e_sigma
    k_t = -(-rows // 4) + 2                                          # W^T u: the 4 waves stride the rows, then the 4 partial sums
    t = w.T @ u
    et = k_t * U * (aw.T @ u.abs())
    nt = max(float(t.norm()), SN_EPS)
    v1 = t / nt
    ev = et / nt + v1.abs() * (float(et.norm()) / nt + 2 * U)        # | |t + dt| - |t| | <= |dt|
    s = w @ v1
    es = aw @ ev + k_wv * U * (aw @ v1.abs())
    ns = max(float(s.norm()), SN_EPS)
    u1 = s / ns
    eu = es / ns + u1.abs() * (float(es.norm()) / ns + 2 * U)
    sigma = u1 @ s
    e_sigma = float(es.norm()) + 2 * U * ns
    return u1, v1, sigma, eu, ev, e_sigma


class _SnState:
    """the device buffers of the table, every output guarded"""

    def __init__(self, data):
        hip, _ = _hip()
        self.w, self.u, self.v, self.sigma, self.tmp, items = [], [], [], [], [], []
        for (rows, cols, mis), (w, u, v) in zip(SN_ITEMS, data):
            gw = guarded_from(w, shift=mis)
            gu, gv = guarded_from(u), guarded_from(v)
            gs, gt = Guarded(1), Guarded(rows + cols + 4)            # tmp: rows + cols + 4 floats as the header says
            assert (gw.ptr() % 16 != 0) == bool(mis) and gt.ptr() % 16 == 0 and gv.ptr() % 16 == 0
            items.append(hip.SNItem(gw.ptr(), gu.ptr(), gv.ptr(), gs.ptr(), gt.ptr(), rows, cols))
            for lst, x in ((self.w, gw), (self.u, gu), (self.v, gv), (self.sigma, gs), (self.tmp, gt)):
                lst.append(x)
        self.table = hip.device_table(items)

    def run(self, power_iter):
        hip, L = _hip()
        hip.check(L.ssr_spectral_norm(self.table.data_ptr(), len(SN_ITEMS), max(r for r, _, _ in SN_ITEMS),
                                      max(c for _, c, _ in SN_ITEMS), power_iter, hip.stream_ptr()), "ssr_spectral_norm")

    def intact(self):
        return all(g.margins_intact() for lst in (self.u, self.v, self.sigma, self.tmp, self.w) for g in lst)


def _sn_check(state, inputs, power_iter, tag, twins=True):
    worst = {}
    got_all = []
    for i, ((rows, cols, mis), (w, u, v)) in enumerate(zip(SN_ITEMS, inputs)):
        vec = _sn_vector_path(rows, cols, mis, power_iter)
        # longest chain of W v: 16-byte loads - a lane adds cols / 256 products into each of 4 sums, 2 adds join them, 6 shuffle levels;
        # scalar - a lane adds cols / 64 products, 6 shuffle levels
        k_wv = (-(-cols // 256) + 2 + 6) if vec else (-(-cols // 64) + 6)
        u1, v1, sigma, eu, ev, e_sigma = _sn_reference(w, u, v, k_wv, power_iter)
        gu, gv, gs = state.u[i].t.cpu(), state.v[i].t.cpu(), state.sigma[i].t.cpu()
        if power_iter:
            ru, rv = within(gu, u1, eu)[1], within(gv, v1, ev)[1]
        else:
            ru = rv = 0.0
            assert same_bits(gu, u.float()) and same_bits(gv, v.float())           # eval mode: u and v stay as they are
        rs = within(gs, sigma.reshape(1), float(e_sigma))[1]
        key = f"{rows}x{cols}{'+1' if mis else ''} {'vector' if vec else 'scalar'}"
        worst[key] = max(ru, rv, rs)
        assert ru <= 1.0 and rv <= 1.0 and rs <= 1.0, (tag, key, ru, rv, rs)
        got_all.append((gu.double(), gv.double(), gs.double(), eu, ev, e_sigma))
    assert state.intact()
    for key, r in worst.items():
        note("spectral_norm", f"{tag} {key}: u, v, sigma error / bound", r, 1.0)
    # the misaligned twin against its aligned twin: the same values through the other path, each within its own bound of the truth
    # (only where both started from the same u and v)
    if not twins:
        return
    (ua, va, sa, eua, eva, esa), (ub, vb, sb, eub, evb, esb) = got_all[-2], got_all[-1]
    if power_iter:
        assert bool(((ua - ub).abs() <= eua + eub).all()) and bool(((va - vb).abs() <= eva + evb).all())
    assert float((sa - sb).abs()) <= esa + esb


def test_spectral_norm_power_iteration_twice_then_eval():
    data = _sn_data()
    st = _SnState(data)
    st.run(1)
    _sn_check(st, data, 1, "iter 1")
    # the second call starts from the first call's u and v: its reference is the float64 step from what the device now holds
    after1 = [(w, g_u.t.cpu().double(), g_v.t.cpu().double()) for (w, _, _), g_u, g_v in zip(data, st.u, st.v)]
    for (w, u0, _), (_, u1, _) in zip(data, after1):
        assert w.shape[0] == 1 or not torch.equal(u0, u1)          # (one row: u is +-1 either way)
    st.run(1)
    _sn_check(st, after1, 1, "iter 2", twins=False)
    after2 = [(w, g_u.t.cpu().double(), g_v.t.cpu().double()) for (w, _, _), g_u, g_v in zip(data, st.u, st.v)]
    st.run(0)
    _sn_check(st, after2, 0, "eval  ", twins=False)


def test_spectral_norm_eval_mode_from_given_vectors():
    """power_iter = 0 on vectors that no power iteration produced: sigma = u . (W v) from the stored u and v, which stay bit-unchanged"""
    data = _sn_data(seed=1)
    st = _SnState(data)
    st.run(0)
    _sn_check(st, data, 0, "eval0 ")


# ================================================================================================ 4. ssr_spectral_norm_bwd
# (rows, cols, which pointer sits one float off 16 bytes).  (256, 4608) passes the cap of 64 blocks x 2048 elements: the dot kernel
# loops, and the smaller items get blocks with nothing to do, whose slots must still be written (tmp starts as NaN).
SNB_ITEMS = [(5, 45, None), (1, 48, None), (7, 576, None), (64, 1152, None), (256, 4608, None), (64, 576, None), (64, 576, "dw"),
             (64, 576, "w")]


def _snb_reference(w, u, v, g):
    """float64 autograd through W / sigma with sigma = u . (W v), u and v detached: what torch's spectral-norm hook differentiates"""
    wp = w.clone().requires_grad_(True)
    sigma = u @ (wp @ v)
    ((wp / sigma) * g).sum().backward()
    return wp.grad, float(sigma.detach())


def _snb_run(data):
    hip, L = _hip()
    bufs, items = [], []
    for (rows, cols, mis), (w, u, v, g, dw0, sigma) in zip(SNB_ITEMS, data):
        gw, gg = guarded_from(w, shift=int(mis == "w")), guarded_from(g)
        gdw = guarded_from(dw0, shift=int(mis == "dw"))
        gu, gv, gs = guarded_from(u), guarded_from(v), guarded_from(torch.tensor([sigma]))
        gt = guarded_from(torch.full((hip.SN_BWD_SLOTS,), float("nan")))            # "nothing to zero"
        items.append(hip.SNBwdItem(gg.ptr(), gw.ptr(), gu.ptr(), gv.ptr(), gs.ptr(), gdw.ptr(), gt.ptr(), rows, cols))
        bufs.append((gdw, gt, gw, gg, gu, gv, gs))
    table = hip.device_table(items)
    hip.check(L.ssr_spectral_norm_bwd(table.data_ptr(), len(items), max(r * c for r, c, _ in SNB_ITEMS), hip.stream_ptr()),
              "ssr_spectral_norm_bwd")
    torch.cuda.synchronize()
    return bufs


def test_spectral_norm_backward():
    gen = torch.Generator().manual_seed(2)
    data = []
    for rows, cols, mis in SNB_ITEMS:
        if mis:
            data.append(data[-1])
            continue
        w = (torch.randn(rows, cols, generator=gen) * 0.05).double()
        u = torch.nn.functional.normalize(torch.randn(rows, generator=gen), dim=0).double()
        v = torch.nn.functional.normalize(torch.randn(cols, generator=gen), dim=0).double()
        g = (torch.randn(rows, cols, generator=gen) * 1e-3).double()
        dw0 = (torch.randn(rows, cols, generator=gen) * 1e-2).double()               # dw starts non-zero: the kernel accumulates
        data.append((w, u, v, g, dw0, float(np.float32(float(u @ (w @ v))))))
    runs = [_snb_run(data), _snb_run(data)]
    gx = grid_for(max(r * c for r, c, _ in SNB_ITEMS), SN_BWD_PER_BLOCK, SN_BWD_CAP)
    assert gx == SN_BWD_CAP                                                          # the largest item does pass the cap
    for i, ((rows, cols, mis), (w, u, v, g, dw0, sigma32)) in enumerate(zip(SNB_ITEMS, data)):
        n = rows * cols
        ref, sigma = _snb_reference(w, u, v, g)
        # <dW_sn, W>: 16-byte loads when n % 4 == 0 and dw_sn, w are aligned - a thread adds ceil(n / 4 / (gx * 256)) products into each of 4
        # sums, 2 adds join them; scalar otherwise - ceil(n / (gx * 256)) products; then the block reduction (6 + 2 levels) and the gx
        # slots added in index order
        per_thread = -(-(n // 4) // (gx * 256)) + 2 if (n % 4 == 0 and mis != "w") else -(-n // (gx * 256))
        k_dot = per_thread + 6 + 2 + gx
        e_dot = k_dot * U * float((g * w).abs().sum())
        term1, term2 = g.abs() / abs(sigma), (float((g * w).sum()) / sigma ** 2) * torch.outer(u, v).abs()
        # per element 4 roundings (1 / sigma, the two products and the difference; sigma itself is handed over rounded to fp32) relative to
        # |dW_sn| / sigma + |coef u_i v_j|, the error of the dot product through coef = dot / sigma^2, and the rounding of the sum
        # stored into the non-zero dw at its own magnitude
        want = dw0 + ref
        bound = 4 * U * (term1 + term2.abs()) + e_dot / sigma ** 2 * torch.outer(u, v).abs() + U * want.abs()
        got = runs[0][i][0].t.cpu().view(rows, cols)
        err, ratio = within(got, want, bound)
        path = "scalar" if (cols % 4 or mis == "dw") else "vector"
        note("spectral_norm_backward", f"{rows}x{cols} {path}{' (' + mis + ' misaligned)' if mis else ''}: error / bound", ratio, 1.0)
        assert ratio <= 1.0, (rows, cols, mis, err, ratio)
        assert same_bits(runs[0][i][0].t, runs[1][i][0].t)                           # two runs: bit-identical
        assert all(b.margins_intact() for run in runs for b in run[i])
        assert bool(torch.isfinite(runs[0][i][1].t).all())                           # every slot was written
        for b, src in zip(runs[0][i][2:], (w, g, u, v, torch.tensor([sigma32]))):    # the inputs are only read
            assert same_bits(b.t, src.reshape(-1).float())


# ================================================================================================ 5. ssr_adam_step (+ fused EMA)
ADAM_EPS = 1e-8


def bias_correction_term(beta, t):
    """The port's known deviation from torch in 1 - beta^t: the kernel raises the fp32-ROUNDED beta to the power t in fp32 (powf, one
    rounding) and subtracts in fp32 (one more); torch uses Python doubles.  Relative to 1 - beta^t:
    (|beta_f32^t - beta^t| + U beta_f32^t) / (1 - beta^t) + U"""
    bf = float(np.float32(beta))
    return (abs(bf ** t - beta ** t) + U * bf ** t) / (1.0 - beta ** t) + U


def _adam_reference(p, g, m, v, ema, lr, t, betas, scale, decay):
    """torch.optim.Adam (single tensor, weight_decay 0, amsgrad off) in float64, bias corrections from the Python doubles, followed by
    BasicSR's model_ema: ema * decay + p * (1 - decay)"""
    b1, b2 = betas
    g = g * scale
    m1 = m + (g - m) * (1 - b1)                                   # exp_avg.lerp_(grad, 1 - beta1)
    v1 = v * b2 + (1 - b2) * g * g                                # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    denom = v1.sqrt() / math.sqrt(bc2) + float(np.float32(ADAM_EPS))      # (torch adds eps as a scalar of the tensor's type)
    upd = (lr / bc1) * (m1 / denom)
    p1 = p - upd
    e1 = ema * decay + p1 * (1 - decay) if ema is not None else None
    # ---- bounds, per element
    em = 3 * U * torch.maximum(m.abs(), g.abs())                  # m: the difference, the product, the sum (and beta1 rounded to fp32)
    ev = 4 * U * torch.maximum(v, g * g)                          # v: v beta2, (1 - beta2) g, . g, the sum (and beta2 rounded to fp32)
    # the update's relative error: 8 roundings (sqrt v, sqrt bc2, their quotient, + eps, m / denom, lr / bc1, the product, and the
    # reciprocal-free division of lr) plus the bias-correction terms (bc1 in full, bc2 through a square root); and the errors of the
    # moments themselves carried through d upd / d m = step / denom and d upd / d sqrt(v) = upd / (denom sqrt(bc2)), with
    # |sqrt(v + e) - sqrt(v)| <= e / (sqrt(v) + sqrt(max(v - e, 0))) (0 where v = e = 0)
    rel = 8 * U + bias_correction_term(b1, t) + 0.5 * bias_correction_term(b2, t)
    dsq = ev / (v1.sqrt() + (v1 - ev).clamp_min(0).sqrt()).clamp_min(1e-300)
    eupd = upd.abs() * rel + (lr / bc1) / denom * em + upd.abs() / denom * dsq / math.sqrt(bc2)
    ep = U * p1.abs() + eupd                                      # half an ulp of |p| for the final subtraction
    # ema: the two products and the sum (decay rounded to fp32 moves both coefficients by less than U / 2), on top of p's own error
    ee = 3 * U * torch.maximum(ema.abs(), p1.abs()) + (1 - decay) * ep if ema is not None else None
    return (p1, m1, v1, e1), (ep, em, ev, ee), upd


def _adam_state(n, seed, moments=True):
    """gradients with magnitudes log-uniform over 1e-8 .. 1, about 1 % exact zeros; every 97th element has m = v = g = 0"""
    g = torch.Generator().manual_seed(seed)
    grad = 10 ** (torch.rand(n, generator=g) * 8 - 8) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    grad[torch.rand(n, generator=g) < 0.01] = 0.0
    s = {"param": torch.randn(n, generator=g) * 0.05, "grad": grad, "ema": torch.randn(n, generator=g) * 0.05}
    if moments:
        s["m"] = 10 ** (torch.rand(n, generator=g) * 8 - 8) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        s["v"] = 10 ** (torch.rand(n, generator=g) * 16 - 16)
    else:
        s["m"], s["v"] = torch.zeros(n), torch.zeros(n)
    for k in ("grad", "m", "v"):
        s[k][96::97] = 0.0
    return s


def _fresh_grad(n, seed):
    return _adam_state(n, seed)["grad"]


def _adam_launch(dev, lr, step, betas, scale, decay, with_ema):
    hip, L = _hip()
    a = hip.AdamArgs(dev["param"].ptr(), dev["grad"].ptr(), dev["m"].ptr(), dev["v"].ptr(), dev["ema"].ptr() if with_ema else None,
                     dev["param"].n, lr.ptr(), step.data_ptr(), betas[0], betas[1], ADAM_EPS, decay, scale)
    hip.check(L.ssr_adam_step(C.byref(a), hip.stream_ptr()), "ssr_adam_step")


def _adam_check(tag, dev, before, lr32, t, betas, scale, decay, with_ema):
    b64 = {k: x.double() for k, x in before.items()}
    (p1, m1, v1, e1), (ep, em, ev, ee), upd = _adam_reference(b64["param"], b64["grad"], b64["m"], b64["v"], b64["ema"] if with_ema else None,
                                                               lr32, t, betas, scale, decay)
    got = {k: dev[k].t.cpu() for k in dev}
    res = {"m": within(got["m"], m1, em)[1], "v": within(got["v"], v1, ev)[1], "param": within(got["param"], p1, ep)[1]}
    if with_ema:
        res["ema"] = within(got["ema"], e1, ee)[1]
    else:
        assert same_bits(got["ema"], before["ema"])               # ema = NULL: the arena handed to other calls stays as it is
    assert same_bits(got["grad"], before["grad"])
    dead = (before["grad"] == 0) & (before["m"] == 0) & (before["v"] == 0)
    assert int(dead.sum()) >= 1 or dev["param"].n < 97
    assert torch.equal(ibits(got["param"])[dead], ibits(before["param"])[dead])     # m = v = g = 0: an update of exactly 0
    assert bool((got["m"][dead] == 0).all()) and bool((got["v"][dead] == 0).all())
    assert all(x.margins_intact() for x in dev.values())
    for k, r in res.items():
        note("adam_step", f"{tag}: {k} error / bound", r, 1.0)
        assert r <= 1.0, (tag, k, r)


ADAM_CASES = [(betas, step0, 100003, 0.125, True) for betas in ((0.9, 0.99), (0.9, 0.999)) for step0 in (0, 1, 9, 999, 99999)] + [
    ((0.9, 0.99), 0, 1, 1.0, True), ((0.9, 0.999), 9, 1, 0.125, False),
    ((0.9, 0.99), 1, 100003, 1.0, False), ((0.9, 0.999), 0, 100003, 1.0, True),
    ((0.9, 0.99), 9, past_cap(ADAM_PER_BLOCK, ADAM_CAP), 1.0, True), ((0.9, 0.999), 999, past_cap(ADAM_PER_BLOCK, ADAM_CAP), 0.125, False)]


@pytest.mark.parametrize("betas,step0,n,scale,with_ema", ADAM_CASES,
                         ids=[f"b2={b[1]}-step{s}-n{n}-scale{sc}-{'ema' if e else 'noema'}" for b, s, n, sc, e in ADAM_CASES])
def test_adam_step_against_float64_adam(betas, step0, n, scale, with_ema):
    decay, lr = 0.999, 1e-4
    before = _adam_state(n, seed=step0 + n)
    dev = {k: guarded_from(x) for k, x in before.items()}
    glr = guarded_from(torch.tensor([lr]))
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    _adam_launch(dev, glr, step, betas, scale, decay, with_ema)
    assert int(step.item()) == step0 + 1
    _adam_check(f"b2={betas[1]} t={step0 + 1} n={n}", dev, before, float(np.float32(lr)), step0 + 1, betas, scale, decay, with_ema)


def test_adam_three_consecutive_steps_from_zero_moments():
    n, betas, decay, lr, scale = 100003, (0.9, 0.99), 0.999, 2e-4, 0.5
    before = _adam_state(n, seed=4, moments=False)
    dev = {k: guarded_from(x) for k, x in before.items()}
    glr = guarded_from(torch.tensor([lr]))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in (1, 2, 3):
        if t > 1:                                                  # a fresh gradient; the state is what the device holds
            dev["grad"].t.copy_(_fresh_grad(n, 40 + t))
        before = {k: x.t.cpu().clone() for k, x in dev.items()}
        _adam_launch(dev, glr, step, betas, scale, decay, True)
        _adam_check(f"consecutive t={t}", dev, before, float(np.float32(lr)), t, betas, scale, decay, True)
    assert int(step.item()) == 3
