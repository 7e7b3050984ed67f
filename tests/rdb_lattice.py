"""The fused ResidualDenseBlock kernels (csrc/rdb_fwd.hip: 8 x 8 tiles, csrc/rdb_tile.hip: 8 x 16 tiles) against a float64 restatement of
the contract of ssr_rdb_desc (include/ssr_hip.h): cases, data, references and the runner through the C ABI (no test functions:
tests/test_rdb_lattice_host.py checks this module on the CPU, tests/test_gpu_rdb_exact.py holds the kernels to it).

A lattice cannot survive five chained stages - x_k passes through fl(0.2f v) and a bf16 store - but it survives ONE stage if the stages
before it hand over lattice values.  An exact case puts one stage under test:

  forward, stage k     x holds integers 0..15.  conv_j, j < k, is a "moved delta": output channel o copies ONE input channel through ONE
                       tap (off-centre taps included), scaled by 1 or 1/2, plus a positive bias: x_j is positive, exactly known, a
                       bf16 number, different at every pixel - and zero outside the image, which a kernel that leaves lrelu(b) in an
                       out-of-image halo pixel gets wrong at the edge pixels of stage k.  conv_k is dense and signed, multiples of 1/8
                       up to 2 with such a bias: its pre-activation is an fp32 number in every summation order.  k < 5: the stored
                       value is bf16(max(v, fl(0.2f v))); k = 5: bf16(alpha5 (conv5 + b5) + beta1 x + beta2 r2) with powers of two.
  backward, slice k    the same on the gather form (ParamStore.add_rdb_gather): d_out and r2 hold integers 0..15, the masks of the slices
                       j > k are positive, the weight blocks W_i[:, block_j] that feed them are moved deltas, every block W_i[:, block_k],
                       i > k, is dense and signed (conv5's divided by a5 = 1/4, which the packing folds back in).  The mask of slice k is
                       mixed and holds planted +0, -0 and the smallest bf16 subnormal of either sign: slope 1 where m > 0 as a real number,
                       0.2f elsewhere (torch's leaky_relu_backward; csrc/common.h: lrelu_mask_lo / lrelu_mask_hi).

Exactness condition, asserted for every case: all operands are multiples of 2^-4, so every term is a multiple of the quantum 2^-8 (times
alpha5 at stage 5), and sum |terms| (bias and residuals included) stays below 2^24 quanta for the worst element.

A teacher-forced case has normal weights, biases and inputs of both signs and the real scales (0.2 | 1, and 0.04 | 0.2 with r2); every
stored stage is recomputed in float64 from the DEVICE's own inputs of that stage (x1..x_{k-1} / dpre and masks as stored) with the weights
as the bf16 numbers the packing produces (bf16(w); bf16(fl(a5 w)) for conv5 in the gather tables), and held to `criterion`:
oracle/layerwise.py::Report.add + check_bf16 for one tensor - one bf16 ulp at most (differences below 1e-5 max|ref|, the cancellation
noise of a near-zero fp32 sum, do not count as ulps, as there), at most max(1, 2e-3 numel) elements differing at all, mean |error| at
most 1e-5 max|ref|.  The cap is a condition, not a measurement: an fp32 F.conv2d (another summation order) meets it against float64 on
every committed case (tests/test_rdb_lattice_host.py)."""
import ctypes as C
import zlib
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace

import torch
import torch.nn.functional as F

NF, GC, CD = 64, 32, 192
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))          # the fp32 number 0.2f, as a double
QUANTUM_BITS = 8
MAX_N = 3
# (H, W): below one tile, the whole image inside the halo (5 x 5), one tile of each kernel, one tile plus one pixel each way, ragged
SHAPES = [(1, 1), (1, 9), (3, 5), (5, 5), (6, 11), (8, 8), (8, 16), (9, 17), (16, 9), (19, 27)]
NHW = [(1, h, w) for h, w in SHAPES] + [(3, 3, 5), (3, 9, 17), (3, 19, 27)]
TILES = (8, 16)
# exact epilogues: powers of two
EXACT_FWD = dict(alpha5=0.25, beta1=0.5, beta2=0.5)
EXACT_BWD = dict(a5=0.25, beta1=0.5, beta2=1.0)
# the engine's epilogues (engine.rdb_epilogue): plain RDB | the one that carries the RRDB's residual
TEACHER = {"plain": dict(alpha5=0.2, beta1=1.0, r2=False, beta2=0.0), "rrdb": dict(alpha5=0.04, beta1=0.2, r2=True, beta2=1.0)}
SPECIAL_BITS = (0x0000, -0x8000, 0x0001, -0x7FFF)              # +0, -0, +-smallest subnormal, as int16


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def _gen(*parts):
    return torch.Generator().manual_seed(_seed(*parts))


def cin_of(j):
    return NF + (j - 1) * GC


def cout_of(j):
    return GC if j < 5 else NF


def block(j):
    """channels of x_j inside cat(x, x1..x4): j = 0 is the block input"""
    return slice(0, NF) if j == 0 else slice(NF + (j - 1) * GC, NF + j * GC)


def has_r2(N, H, W):
    """exact cases: r2 on every other shape, the other way round at N = 3 (both epilogues on sub-tile and on ragged shapes)"""
    return (SHAPES.index((H, W)) % 2 == 0) != (N == 3)


# ================================================================================================ number formats
def r32(t):
    """one fp32 rounding of a float64 tensor"""
    return t.float().double()


def bf16_rne(v):
    """float64 tensor of fp32 numbers -> bfloat16, round to nearest even on the raw bits (finite values)"""
    bits = v.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16).view(torch.bfloat16)


def lrelu32(v):
    """max(v, fl(0.2f v)) on fp32 numbers held in float64: what v_max_f32 of csrc/common.h: lrelu_max computes"""
    return torch.maximum(v, r32(v * SLOPE))


def stored(v):
    """bf16 store of fp32 numbers, back in float64"""
    return bf16_rne(v).double()


def slope_of(m, mut=None):
    """LeakyReLU' from the saved output m (float64 of bf16 values): 1 where m > 0 as a real number, 0.2f elsewhere"""
    pos = m > 0
    if mut == "one_at_plus_zero":
        pos = pos | ((m == 0) & ~torch.signbit(m))
    elif mut == "subnormal_as_negative":
        pos = pos & (m >= 2.0 ** -126)
    return pos


def masked32(acc, m, mut=None):
    return torch.where(slope_of(m, mut), acc, r32(acc * SLOPE))


# ================================================================================================ float64 contract
def conv(x, w, b=None):
    return F.conv2d(x, w, b, padding=1)


def conv_t(dy, w):
    """dL/dx of conv(x, w) given dL/dy; w = the forward weight's [Cout, slice of Cin, 3, 3]"""
    return F.conv_transpose2d(dy, w, padding=1)


def forward_stage(k, feats, w, b, halo_bias=None):
    """pre-activation of conv_k over cat(feats) and sum |terms| + |bias|.  halo_bias (mutation): {j: b_j} - x_j keeps lrelu(b_j) in the
    ring of pixels outside the image instead of the zero padding"""
    x = torch.cat(feats, 1)
    if halo_bias:
        xp = F.pad(x, (1, 1, 1, 1))
        ring = torch.ones_like(xp[:1, :1], dtype=torch.bool)
        ring[..., 1:-1, 1:-1] = False
        for j, bj in halo_bias.items():
            if j < k:
                xp[:, block(j)] = torch.where(ring, lrelu32(bj.double()).view(1, -1, 1, 1), xp[:, block(j)])
        pre = F.conv2d(xp, w, b)
    else:
        pre = conv(x, w, b)
    mag = conv(x.abs(), w.abs(), b.abs())
    return pre, mag


def forward64(x, W, B, ep, r2=None, given=None, value=lambda pre: torch.where(pre > 0, pre, pre * SLOPE), round_=None, halo_bias=None,
              b5_outside=False):
    """The dense block of ssr_rdb_desc, forward: -> {k: (value, pre, mag)}, k = 1..5, float64 NCHW.  `given` {j: x_j}: the inputs of the later
    stages (teacher forcing); otherwise round_(value) is handed on.  W, B: {j: float64 OIHW / [Cout]}"""
    feats, out = [x], {}
    for k in range(1, 6):
        pre, mag = forward_stage(k, feats, W[k], B[k], halo_bias)
        if k < 5:
            val = value(pre)
            feats.append(given[k] if given is not None else round_(val))
        else:
            a5, b1, b2 = (float(torch.tensor(ep[n], dtype=torch.float32)) for n in ("alpha5", "beta1", "beta2"))
            if b5_outside:
                pre = pre - B[5].view(1, -1, 1, 1) + B[5].view(1, -1, 1, 1) / a5
            val, mag = a5 * pre + b1 * x, a5 * mag + abs(b1) * x.abs()
            if r2 is not None:
                val, mag = val + b2 * r2, mag + abs(b2) * r2.abs()
        out[k] = (val, pre, mag)
    return out


def backward64(d_out, masks, W, ep, r2=None, given=None, value=None, round_=None, shift=None):
    """The gather-form backward: slice j <- sum_{i > j} conv_t(dpre_i, W_i[:, block_j]) + conv_t(d_out, W_5[:, block_j]), W_5 with a5
    folded in, times lrelu'(masks[j]) for j = 1..4; slice 0 adds beta1 d_out + beta2 r2.  -> {j: (value, acc, mag)}, j = 4..0.
    `given` {j: dpre_j} for teacher forcing; shift (mutation) = (i, j): conv i's segment of slice j reads one block further"""
    value = value or (lambda acc, m: torch.where(m > 0, acc, acc * SLOPE))
    dpre, out = {}, {}
    for j in (4, 3, 2, 1, 0):
        acc = mag = 0.0
        for i in range(j + 1, 6):
            src = d_out if i == 5 else dpre[i]
            blk = block(j)
            if shift == (i, j):
                off = GC if blk.stop + GC <= cin_of(i) else -GC
                blk = slice(blk.start + off, blk.stop + off)
            acc = acc + conv_t(src, W[i][:, blk])
            mag = mag + conv_t(src.abs(), W[i][:, blk].abs())
        if j > 0:
            val = value(acc, masks[j])
            dpre[j] = given[j] if given is not None else round_(val)
        else:
            b1, b2 = (float(torch.tensor(ep[n], dtype=torch.float32)) for n in ("beta1", "beta2"))
            val, mag = acc + b1 * d_out, mag + abs(b1) * d_out.abs()
            if r2 is not None:
                val, mag = val + b2 * r2, mag + abs(b2) * r2.abs()
        out[j] = (val, acc, mag)
    return out


# ================================================================================================ exact cases
@dataclass(frozen=True)
class Exact:
    direction: str            # "fwd": k = stage 1..5 | "bwd": k = slice 4..0
    k: int
    N: int
    H: int
    W: int

    @property
    def name(self):
        return f"{self.direction}{self.k}-{self.N}x{self.H}x{self.W}"

    @property
    def r2(self):
        return has_r2(self.N, self.H, self.W)


EXACT_CASES = [Exact(d, k, n, h, w) for d, ks in (("fwd", (1, 2, 3, 4, 5)), ("bwd", (4, 3, 2, 1, 0))) for (n, h, w) in NHW for k in ks]


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _signed_eighths(shape, gen):
    """+-{1/8 .. 2}: never zero, so every tap, channel and chunk carries data"""
    return _ints(shape, 1, 16, gen) * (_ints(shape, 0, 1, gen) * 2 - 1) / 8


def _delta(cout, cin, gen):
    w = torch.zeros(cout, cin, 3, 3, dtype=torch.float64)
    c, t, s = torch.randint(0, cin, (cout,), generator=gen), torch.randint(0, 9, (cout,), generator=gen), torch.randint(0, 2, (cout,), generator=gen)
    w[torch.arange(cout), c, t // 3, t % 3] = 2.0 ** -s.double()
    return w


@lru_cache(maxsize=None)
def exact_weights(direction, k):
    """-> (W, B): {j: float64 OIHW}, {j: float64 [Cout]} of conv1..5 as the reference model stores them (shared: do not modify)"""
    g = _gen("exact-w", direction, k)
    W, B = {}, {}
    if direction == "fwd":
        for j in range(1, 6):
            if j == k:
                W[j], B[j] = _signed_eighths((cout_of(j), cin_of(j), 3, 3), g), _ints((cout_of(j),), -8, 8, g) / 4
            else:
                W[j], B[j] = _delta(cout_of(j), cin_of(j), g), _ints((cout_of(j),), 1, 3, g) / 2
        return W, B
    a5 = EXACT_BWD["a5"]
    for j in range(1, 6):
        W[j], B[j] = torch.zeros(cout_of(j), cin_of(j), 3, 3, dtype=torch.float64), torch.zeros(cout_of(j), dtype=torch.float64)
    for j in (4, 3, 2, 1, 0):
        blk = block(j)
        n = blk.stop - blk.start
        if j == k:
            for i in range(j + 1, 6):
                W[i][:, blk] = _signed_eighths((cout_of(i), n, 3, 3), g) / (a5 if i == 5 else 1.0)
            continue
        src = torch.randint(j + 1, 6, (n,), generator=g)             # one later conv, one of its channels, one tap per channel of the slice
        for c in range(n):
            i = int(src[c])
            o, t, s = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (cout_of(i), 9, 2))
            W[i][o, blk.start + c, t // 3, t % 3] = 2.0 ** -s / (a5 if i == 5 else 1.0)
    return W, B


@lru_cache(maxsize=None)
def _exact_data(direction, k, H, W):
    g = _gen("exact-x", direction, k, H, W)
    shape = (MAX_N, NF, H, W)
    if direction == "fwd":
        return dict(x=_ints(shape, 0, 15, g), r2=_ints(shape, -15, 15, g))
    out = dict(d_out=_ints(shape, 0, 15, g), r2=_ints(shape, 0, 15, g), masks={})
    for j in range(1, 5):
        mshape = (MAX_N, GC, H, W)
        m = _ints(mshape, 1, 6, g) / 2
        if j <= k:
            m = m * (_ints(mshape, 0, 1, g) * 2 - 1)
        bits = m.bfloat16().view(torch.int16).reshape(MAX_N, -1).clone()
        if j == k:
            for n in range(MAX_N):
                at = torch.randperm(bits.shape[1], generator=g)[:len(SPECIAL_BITS)]
                bits[n, at] = torch.tensor(SPECIAL_BITS, dtype=torch.int16)
        out["masks"][j] = bits.view(mshape).view(torch.bfloat16)
    return out


def exact_data(case):
    """fwd: x, r2 float64 [N, 64, H, W]; bwd: d_out, r2 and masks {j: bfloat16 [N, 32, H, W]} (image n is image n of every batch)"""
    d = _exact_data(case.direction, case.k, case.H, case.W)
    out = {key: (v[:case.N] if key != "masks" else {j: m[:case.N] for j, m in v.items()}) for key, v in d.items()}
    if not case.r2:
        out["r2"] = None
    return out


def _on_grid(t, what):
    assert torch.equal((t * 16).round(), t * 16), f"{what}: not on the 2^-4 grid"


def exact_expected(case, W=None, mut=None):
    """-> ({stage or slice: float64 NCHW of the bf16 numbers the kernel must store, for every stage up to the one under test},
    margin of the stage under test).  Asserts the exactness condition.  W and mut are the mutations of the host test (there the
    assertions on the handed-over values are the same, those on the mutated sums are skipped)."""
    if W is None and mut is None:
        return _exact_expected(case)
    return _exact_expected_of(case, W, mut)


@lru_cache(maxsize=None)
def _exact_expected(case):
    return _exact_expected_of(case, None, None)


def _exact_expected_of(case, W, mut):
    strict = W is None and mut is None
    W0, B = exact_weights(case.direction, case.k)
    W = W or W0
    d = exact_data(case)
    k = case.k
    if case.direction == "fwd":
        res = forward64(d["x"], W, B, EXACT_FWD, d["r2"], value=lrelu32, round_=stored,
                        halo_bias={j: B[j] for j in range(1, 5)} if mut == "halo_bias" else None, b5_outside=mut == "b5_outside")
        order, quantum = list(range(1, k + 1)), 2.0 ** -QUANTUM_BITS * (EXACT_FWD["alpha5"] if k == 5 else 1.0)
        for j in range(1, k):
            _on_grid(W[j], "delta weight")
    else:
        a5 = EXACT_BWD["a5"]
        Wf = {i: (w * a5 if i == 5 else w) for i, w in W.items()}
        res = backward64(d["d_out"], {j: m.double() for j, m in d["masks"].items()}, Wf, EXACT_BWD, d["r2"],
                         value=lambda acc, m: masked32(acc, m, mut if mut in ("one_at_plus_zero", "subnormal_as_negative") else None),
                         round_=stored, shift=(5, k) if mut == "shift_segment" else None)
        order, quantum = list(range(4, k - 1, -1)), 2.0 ** -QUANTUM_BITS
    want = {}
    for j in order:
        val, pre, mag = res[j]
        want[j] = stored(val)
        if strict:
            _on_grid(W[j] if case.direction == "fwd" else torch.cat([Wf[i][:, block(j)].flatten() for i in range(j + 1, 6)]), f"{case.name} weights {j}")
            assert float(mag.max()) / quantum < 2.0 ** 24, f"{case.name} stage {j}: the sum is not exact in every order"
            assert torch.equal(r32(pre), pre), f"{case.name} stage {j}: the accumulator is no fp32 number"
            assert j not in (0, 5) or torch.equal(r32(val), val), f"{case.name} stage {j}: the epilogue's sum is no fp32 number"
            if j != k:                            # a handed-over stage: positive, exactly known, a bf16 number
                assert torch.equal(want[j], val) and bool((val >= 0).all()), f"{case.name}: stage {j} does not hand over lattice values"
                _on_grid(val, f"{case.name} stage {j}")
    margin = float(res[k][2].max()) / quantum / 2.0 ** 24
    return want, margin


# ================================================================================================ mutations
def without_tap(case, conv_j, chunk, ty, tx):
    W = {j: w.clone() for j, w in exact_weights(case.direction, case.k)[0].items()}
    W[conv_j][:, chunk, ty, tx] = 0.0
    return W


# (what, the committed case whose exact comparison catches it, the arguments of exact_expected that make the mistake on the reference side)
MUTATIONS = [
    ("one tap of one chunk dropped (forward conv3, chunk 1, tap (0, 2))", Exact("fwd", 3, 1, 9, 17),
     lambda c: dict(W=without_tap(c, 3, slice(32, 64), 0, 2))),
    ("one tap of one chunk dropped (backward slice 2, conv4's segment, tap (1, 0))", Exact("bwd", 2, 1, 9, 17),
     lambda c: dict(W=without_tap(c, 4, block(2), 1, 0))),
    ("one tap of one 16-channel half chunk of conv5 dropped", Exact("fwd", 5, 1, 8, 16), lambda c: dict(W=without_tap(c, 5, slice(176, 192), 2, 2))),
    ("lrelu(bias) kept in out-of-image halo pixels (stage 2 reads x1)", Exact("fwd", 2, 1, 3, 5), lambda c: dict(mut="halo_bias")),
    ("lrelu(bias) kept in out-of-image halo pixels (conv5, whole image inside the halo)", Exact("fwd", 5, 1, 5, 5), lambda c: dict(mut="halo_bias")),
    ("lrelu(bias) kept in out-of-image halo pixels (tile edge inside the image)", Exact("fwd", 4, 3, 9, 17), lambda c: dict(mut="halo_bias")),
    ("mask slope 1 at +0", Exact("bwd", 2, 1, 6, 11), lambda c: dict(mut="one_at_plus_zero")),
    ("mask slope 0.2 at a positive subnormal", Exact("bwd", 2, 1, 6, 11), lambda c: dict(mut="subnormal_as_negative")),
    ("mask slope 1 at +0, 1 x 1 image", Exact("bwd", 4, 1, 1, 1), lambda c: dict(mut="one_at_plus_zero")),
    ("conv5's accumulator started at b5 outside the alpha5 scale", Exact("fwd", 5, 1, 1, 1), lambda c: dict(mut="b5_outside")),
    ("channel offset of conv5's gather segment shifted by one block", Exact("bwd", 2, 1, 9, 17), lambda c: dict(mut="shift_segment")),
    ("channel offset of conv5's gather segment shifted by one block (slice 0)", Exact("bwd", 0, 1, 3, 5), lambda c: dict(mut="shift_segment")),
]


# ================================================================================================ teacher-forced cases
@lru_cache(maxsize=None)
def teacher_weights():
    g = _gen("teacher-w")
    W = {j: (torch.randn(cout_of(j), cin_of(j), 3, 3, generator=g) * 0.03) for j in range(1, 6)}
    B = {j: (torch.randn(cout_of(j), generator=g) * 0.1) for j in range(1, 6)}
    return W, B                                   # fp32, as the state_dict holds them


@lru_cache(maxsize=None)
def _teacher_data(H, W):
    g = _gen("teacher-x", H, W)
    return {n: torch.randn(MAX_N, NF, H, W, generator=g).bfloat16().double() for n in ("x", "r2", "d_out", "d_r2")}


def teacher_data(N, H, W):
    return {k: v[:N] for k, v in _teacher_data(H, W).items()}


def packed_values(W, a5=None):
    """the bf16 numbers in the packed tables, float64: bf16(w) (ssr_pack_weights); a5 given: conv5 as bf16(fl(a5 w)) (ssr_pack_dgrad_gather)"""
    out = {j: w.float().bfloat16().double() for j, w in W.items()}
    if a5 is not None:
        out[5] = (W[5].float() * torch.tensor(a5, dtype=torch.float32)).bfloat16().double()
    return out


def bf16_ulp(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-38))) - 7)


def criterion(got, ref64):
    """oracle/layerwise.py: Report.add + check_bf16 for one tensor.  got: float64 of the stored bf16 numbers -> (ok, stats)"""
    ref = ref64.float().bfloat16().double()
    scale = float(ref.abs().max()) + 1e-30
    d = (got - ref).abs()
    big = d > 1e-5 * scale
    ulps = float((d[big] / bf16_ulp(torch.maximum(ref.abs(), got.abs())[big])).max()) if bool(big.any()) else 0.0
    ndiff, mean = int((d > 0).sum()), float(d.mean()) / scale
    cap = max(1, int(2e-3 * d.numel()))
    finite = bool(torch.isfinite(got).all())
    return finite and ulps <= 1.0 and ndiff <= cap and mean <= 1e-5, dict(ulps=ulps, differing=ndiff, numel=d.numel(), mean=mean)


def teacher_forward_check(x, r2, ep, slices, out):
    """slices {j: float64 x_j as stored}, out float64 -> {stage: (ok, stats)}: every stage from the stored inputs of that stage"""
    W, B = teacher_weights()
    Wp, Bd = packed_values(W), {j: b.double() for j, b in B.items()}
    ref = forward64(x, Wp, Bd, ep, r2 if ep["r2"] else None, given=slices)
    got = dict(slices)
    got[5] = out
    return {k: criterion(got[k], ref[k][0]) for k in range(1, 6)}


def teacher_backward_check(d_out, r2, ep, masks, dpre, dx):
    W, _ = teacher_weights()
    ref = backward64(d_out, masks, packed_values(W, ep["alpha5"]), ep, r2 if ep["r2"] else None, given=dpre)
    got = dict(dpre)
    got[0] = dx
    return {j: criterion(got[j], ref[j][0]) for j in (4, 3, 2, 1, 0)}


# ================================================================================================ the runner
POISON = 0x7FC5                                   # a bf16 NaN with a payload of its own: poison and sentinel in one


@dataclass(frozen=True)
class Layout:
    """where the views lie: alias = the engine's forms (forward in == slices; backward out == slices), else every view in a buffer of
    its own; per view (coff, channels behind the view): cs = coff + channels + tail"""
    alias: bool = True
    inp: tuple = (0, 0)
    slices: tuple = (0, 0)
    out: tuple = (0, 0)
    mask: tuple = (0, 0)
    r2: tuple = (0, 0)


ENGINE = Layout()
# channel slices: coff in {8, 16}, a cs of its own for every view, none of them 192; r2 and mask at 4 mod 8
SLICED = {
    "fwd": (Layout(True, slices=(8, 8), out=(16, 16), r2=(4, 8)),                                       # cs: 208, 96, 76
            Layout(False, inp=(8, 8), slices=(16, 8), out=(8, 16), r2=(12, 8))),                       # cs: 80, 216, 88, 84
    "bwd": (Layout(True, inp=(8, 8), slices=(16, 16), mask=(12, 8), r2=(4, 4)),                        # cs: 80, 224, 212, 72
            Layout(False, inp=(16, 8), slices=(8, 16), out=(8, 24), mask=(4, 12), r2=(12, 8))),        # cs: 88, 216, 96, 208, 84
}


class Buf:
    """C channels at [coff, coff + C) of a NHWC bf16 buffer of coff + C + tail channels with one pixel row of guard before and after,
    filled with the bit pattern `fill` (int16)"""

    def __init__(self, N, H, W, Cn, place, fill):
        coff, tail = place
        self.coff, self.C, self.cs = coff, Cn, coff + Cn + tail
        self.row = W * self.cs
        n = N * H * W * self.cs
        self.flat = torch.full((n + 2 * self.row,), fill, dtype=torch.int16, device="cuda")
        self.t = self.flat[self.row:self.row + n].view(N, H, W, self.cs)
        self.written = torch.zeros_like(self.flat, dtype=torch.bool)

    def put(self, c0, nchw):
        v = nchw.permute(0, 2, 3, 1)
        v = v if v.dtype == torch.bfloat16 else v.float().bfloat16()
        self.t[..., self.coff + c0:self.coff + c0 + v.shape[-1]] = v.contiguous().view(torch.int16).cuda()
        return self

    def may_write(self, c0, c1):
        self.written[self.row:self.row + self.t.numel()].view(self.t.shape)[..., self.coff + c0:self.coff + c1] = True

    def snapshot(self):
        self.before = self.flat.clone()

    def view(self, hip):
        return hip.View(self.t.data_ptr(), self.cs, self.coff)

    def get(self, c0, c1):
        """float64 NCHW of the stored numbers"""
        return self.t[..., self.coff + c0:self.coff + c1].contiguous().view(torch.bfloat16).cpu().double().permute(0, 3, 1, 2).contiguous()

    def bits(self, c0, c1):
        return self.t[..., self.coff + c0:self.coff + c1].cpu()

    def outside_unchanged(self):
        return bool((self.flat[~self.written] == self.before[~self.written]).all())

    def unchanged(self):
        return torch.equal(self.flat, self.before)


@lru_cache(maxsize=None)
def packed(kind, direction="", k=0, a5=0.0):
    """the project's own packing of one block's weights: ParamStore.pack() for conv1..4, add_repack(conv5, 16), add_rdb_gather(prefix,
    64, 32, a5, ck0=16) - what GeneratorPlan._build_forward / _build_backward hand to the kernels"""
    from satlas_super_resolution_amd import engine, hip
    W, B = teacher_weights() if kind == "teacher" else exact_weights(direction, k)
    names = [f"b.conv{j}" for j in range(1, 6)]
    st = engine.ParamStore([engine.ConvSpec(names[j - 1], cout_of(j), cin_of(j), 3, 1, True, False, dgrad_packed=False) for j in range(1, 6)], hip.BF16)
    sd = {}
    for j in range(1, 6):
        sd[names[j - 1] + ".weight"], sd[names[j - 1] + ".bias"] = W[j].float(), B[j].float()
    st.load_state_dict(sd)
    w5 = st.add_repack("b.conv5", 16)
    st.add_rdb_gather("b", NF, GC, a5, ck0=16)
    st.pack()
    torch.cuda.synchronize()
    fwd = [st.packed_fwd[n] for n in names[:4]] + [w5]
    bwd = [st.gather[("b", j)] for j in (4, 3, 2, 1)] + [st.gather[("b", "k0", 16)]]
    return SimpleNamespace(store=st, fwd=fwd, bwd=bwd, bias=[st.ptr(n + ".bias") for n in names])


def run(direction, tile, pk, ep, t, layout=ENGINE, poison=True, w_next=False, tweak=None):
    """One launch of ssr_rdb_forward / ssr_rdb_backward through the C ABI with a hand-built RdbDesc and the kernel forced.
    t: fwd {x, r2 | None}; bwd {d_out, r2 | None, masks: [N, 128, H, W] bf16 or float64 of x1..x4} (NCHW, CPU).
    poison: the POISON pattern (a NaN) wherever the contract says nothing is read - the stale channels [64, 192) of `slices` before a
    forward, all of `slices` and `out` before a backward, channels [0, 64) of `mask`, every channel outside a view and the guard rows;
    otherwise zeros there (and ones in the stale channels).  tweak(d): edits the descriptor before the launch (refusals).
    -> rc, slices {j: float64 NCHW}, out, slice_bits / out_bits (int16 NHWC), guards_ok (nothing outside the output views changed),
    inputs_ok (in, mask, r2 - and channels [0, 64) of an aliased forward buffer - unchanged), untouched (no buffer changed at all)"""
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    bwd = direction == "bwd"
    src = t["d_out"] if bwd else t["x"]
    N, _, H, Wd = src.shape
    fill = POISON if poison else 0
    mk = lambda Cn, place: Buf(N, H, Wd, Cn, place, fill)      # noqa: E731
    bufs = {}
    if bwd:
        bufs["inp"] = mk(NF, layout.inp).put(0, src)
        bufs["mask"] = mk(CD, layout.mask).put(NF, t["masks"])
        bufs["slices"] = mk(CD, layout.slices)
        bufs["out"] = bufs["slices"] if layout.alias else mk(NF, layout.out)
    else:
        bufs["slices"] = mk(CD, layout.slices)
        if not poison:
            bufs["slices"].put(NF, torch.ones(N, CD - NF, H, Wd))
        bufs["inp"] = bufs["slices"].put(0, src) if layout.alias else mk(NF, layout.inp).put(0, src)
        bufs["out"] = mk(NF, layout.out)
    if t.get("r2") is not None:
        bufs["r2"] = mk(NF, layout.r2).put(0, t["r2"])
    bufs["slices"].may_write(NF, CD)
    bufs["out"].may_write(0, NF)
    for b in bufs.values():
        b.snapshot()
    d = hip.RdbDesc()
    d.dtype, d.N, d.H, d.W = hip.BF16, N, H, Wd
    d.inp, d.slices, d.out = bufs["inp"].view(hip), bufs["slices"].view(hip), bufs["out"].view(hip)
    d.mask = bufs["mask"].view(hip) if bwd else hip.NULL_VIEW
    ws = pk.bwd if bwd else pk.fwd
    for j in range(5):
        d.w[j] = ws[j].data_ptr()
        d.bias[j] = None if bwd else pk.bias[j]
        if w_next:
            d.w_next[j], d.w_next_bytes[j] = ws[j].data_ptr(), ws[j].numel() * 2
    d.alpha5, d.beta1 = (1.0 if bwd else ep["alpha5"]), ep["beta1"]
    d.r2, d.beta2 = (bufs["r2"].view(hip), ep["beta2"]) if "r2" in bufs else (hip.NULL_VIEW, 0.0)
    d.tile = tile
    assert lib.ssr_rdb_tile_of(C.byref(d)) == tile, "the forced kernel is the one that runs"
    if tweak:
        tweak(d)
    rc = (lib.ssr_rdb_backward if bwd else lib.ssr_rdb_forward)(C.byref(d), hip.stream_ptr())
    torch.cuda.synchronize()
    sl, ob = bufs["slices"], bufs["out"]
    ins = [b for n, b in bufs.items() if n in ("mask", "r2") or (n == "inp" and b is not sl)]
    return SimpleNamespace(
        rc=rc, slices={j: sl.get(block(j).start, block(j).stop) for j in range(1, 5)}, out=ob.get(0, NF),
        slice_bits=sl.bits(NF, CD), out_bits=ob.bits(0, NF),
        guards_ok=sl.outside_unchanged() and ob.outside_unchanged(), inputs_ok=all(b.unchanged() for b in ins),
        untouched=all(b.unchanged() for b in bufs.values()))


def exact_tensors(case):
    d = exact_data(case)
    if case.direction == "fwd":
        return dict(x=d["x"], r2=d["r2"])
    return dict(d_out=d["d_out"], r2=d["r2"], masks=torch.cat([d["masks"][j] for j in range(1, 5)], 1))


def exact_packed(case):
    return packed("exact", case.direction, case.k, EXACT_BWD["a5"])


def exact_mismatch(case, res):
    """None, or what differs between the launch and the exact targets of every stage up to the one under test"""
    want, margin = exact_expected(case)
    msgs = []
    for j, w in want.items():
        got = res.out if j in (0, 5) else res.slices[j]
        if not torch.equal(got, w):
            bad = ~(got == w)
            first = tuple(int(v) for v in bad.nonzero()[0])
            msgs.append(f"stage {j}: {int(bad.sum())} of {bad.numel()} elements differ, first at (n, c, y, x) = {first}: got {float(got[first])!r}, "
                        f"want {float(w[first])!r}")
    if not res.guards_ok:
        msgs.append("a write outside the output views")
    if not res.inputs_ok:
        msgs.append("an input was written")
    return f"{case.name} (margin {margin:.4f}): " + "; ".join(msgs) if msgs else None
