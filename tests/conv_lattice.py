"""Inputs for which a forward or data-gradient convolution is an EXACT sum, the float64 contract reference with its epilogue as exact
targets, and a runner through the project's own path (no test functions: tests/test_conv_lattice_host.py checks this module on the CPU,
tests/test_gpu_conv_exact.py holds the kernels to it).  The lattices `coarse_lattice`, `split_lattice`, `split_planes` and `rup` are
those of tests/wgrad_lattice.py.

With operands on a dyadic lattice every product is a multiple of one granule 2^-g; while sum |terms| < 2^24 granules every partial sum
of every summation order is an fp32 number, so MFMA accumulation, the K-quarter sums, the ring order and the chunk order must all give
the bits of the float64 sum.  A missing, doubled or misplaced term is a different number, never a rounding.

  coarse  v = a + b / 16      a in +-{1, 2, 3}, b in {-1, 0, 1}: exact in bf16; products are multiples of 2^-8
  split   v = a + b * 2^-9    ssr_split_bf16 gives hi = a, lo = b * 2^-9; products of pieces are multiples of 2^-9 (lo.lo: 2^-18)
  half    v = a + b * 2^-12   a in +-{2, 3}: f16(v) = a, f16(v - a) = b * 2^-12, f16(2^10 v) = 2^10 a and the rest b * 2^-2, no
                              round-to-even tie (a = +-1 is left out: 1 - 2^-12 lies half way between two fp16 numbers); multiples of 2^-12

The term set a kernel is defined to compute, as read from the code:

  bf16, every family; exact fp32 (thin<., 0>, x3r AM = 1, res, pipelined)      x.w on the coarse lattice
  fp32x3, MFMA families (csrc/conv_big_x3.hip: the three MFMAs per tap of conv_bigx3_kernel4; csrc/conv_x3r_core.h; csrc/conv_x3q.hip;
      conv_x3_kernel of csrc/conv.hip; include/ssr_hip.h:31-34)                 xh.wh + xh.wl + xl.wh on the split lattice, lo.lo dropped
  fp32h forward, MFMA families (include/ssr_hip.h:35-45: "a_lo w_hi + a_hi w_lo + a_hi w_hi", the weight pieces those of 2^10 w,
      accumulators x 2^-10; conv_bigh3_kernel4 starts them at 2^10 bias)       the same three terms on fp16 pieces of the half lattice
  conv_thin_f32_kernel<., 1 | 2> (csrc/conv_thin.hip:187-195: w = hi + lo rebuilt in fp32, one fp32 FMA per product with the unsplit x)
                                                                                x.(wh + wl) = x.w, the full product: w on the split / half
                                                                                lattice (so that the lo plane carries data), x = a alone
                                                                                (integers: the products stay on the granule of w)

The exactness condition is asserted for every case by `expected` (never skipped): margin = (sum |terms| + |bias|) / granule / 2^24 < 1
for the worst output element.  fp32h at granule 2^-12 would break it at K = 1728 (192 channels, 3x3): there the weights are thinned (a
fixed share is zero, `keep_share`), K is not shrunk.

The epilogue (include/ssr_hip.h: s0 = alpha act(acc + bias); s1 = s0 + beta1 r1 + beta2 r2 + y_old; y = s1 lrelu'(m)) with bias, r1, r2,
y_old and m on the coarse lattice and alpha, beta1, beta2 powers of two of either sign: everything up to the activation is an fp32
number, the only roundings are fl(0.2f v) on the negative side of LeakyReLU or of the mask and the additions that follow a rounded
value.  One rounded value plus one further term is unique; with two or three further terms the element must be ONE of the fp32
evaluations in which the exact terms meet it in some grouped order: the ordered set partitions of the terms (13 for three).  `finish`
returns the stack of those evaluations; where nothing was rounded they all coincide (asserted) with the float64 value."""
import contextlib
import ctypes as C
import os
import zlib
from dataclasses import dataclass
from functools import lru_cache
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from wgrad_lattice import coarse_lattice, rup, split_lattice, split_planes

GRANULE_BITS = {"coarse": 8, "split": 9, "half": 12}
WSHIFT = 10                                    # SSR_F32H_WSHIFT
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))          # the fp32 number 0.2f, as a double
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
X_GUARD = 8                                    # channels in front of and behind every view


# ================================================================================================ lattices
def half_lattice(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randint(2, 4, shape, generator=gen).double() * (torch.randint(0, 2, shape, generator=gen).double() * 2 - 1)
    b = torch.randint(-1, 2, shape, generator=gen).double()
    return (a + b * 2.0 ** -12).float()


LATTICES = {"coarse": coarse_lattice, "split": split_lattice, "half": half_lattice}


def half_planes(x, shift=0):
    """hi = f16(2^shift x), lo = f16(2^shift x - hi), both x 2^-shift: the fp16 split of include/ssr_hip.h (activations: shift 0;
    packed weights: shift 10), round to nearest even"""
    s = x * 2.0 ** shift
    hi = s.to(torch.float16)
    lo = (s - hi.float()).to(torch.float16)
    return hi.float() * 2.0 ** -shift, lo.float() * 2.0 ** -shift


def keep_share(lattice, K):
    """share of the weights that stay non-zero: 1 unless the plain lattice would break the exactness condition at this K (products of
    the half lattice reach 9 = 36864 granules: about 256 of them fit)"""
    return min(1.0, 256.0 / K) if lattice == "half" else 1.0


# ================================================================================================ families, modes, epilogues
# family -> the ssr_conv2d_impl code that reaches it (res cannot be forced: 2 = "not the weight-stationary kernel" leaves it first in line)
IMPL = {"thin": 5, "ws": 1, "big": 4, "bigx3": 4, "x3r": 7, "x3q": 6, "res": 2, "pipelined": 3}
X_SENTINEL = float("nan")                      # what the input guard channels hold: an over-read that reaches an accumulator poisons the output


def arithmetic(family, mode):
    """-> (lattice, pieces): pieces None = one product x.w, "bf16" / "f16" = the three products of the split pieces"""
    if mode in ("bf16", "fp32"):
        return "coarse", None
    if family == "thin":                       # the full product with w = hi + lo rebuilt: w on the mode's lattice (lo != 0), x integer
        return ("split" if mode == "fp32x3" else "half"), None
    return ("split", "bf16") if mode == "fp32x3" else ("half", "f16")


def integer_x(family, mode):
    """the thin kernels of the split modes: x = a alone, so that x.w stays on the granule of w"""
    return family == "thin" and mode in ("fp32x3", "fp32h")


def symbol_prefix(family, mode):
    """how ssr_conv2d_symbol names the family's kernel in this mode"""
    if family == "thin":
        return "conv_thin_kernel<" if mode == "bf16" else "conv_thin_f32_kernel<"
    if family == "bigx3":
        return "conv_bigh3_kernel4<" if mode == "fp32h" else "conv_bigx3_kernel4<"
    if family == "pipelined":
        return {"fp32x3": "conv_x3_kernel<", "fp32h": "conv_h3_kernel<"}.get(mode, "conv_kernel<")
    return {"ws": "conv_ws_kernel<", "big": "conv_big_kernel<", "x3r": "conv_x3r_kernel<", "x3q": "conv_x3q_kernel<", "res": "conv_res_kernel<"}[family]


@dataclass(frozen=True)
class Epilogue:
    act: int = ACT_NONE
    alpha: float = 1.0
    y0: bool = False
    r1: Optional[float] = None            # beta1
    r2: Optional[float] = None            # beta2
    acc: bool = False
    m: bool = False
    m_relu: bool = False
    y1: bool = False


# the VARIANTS of tests/test_gpu_conv_x3.py with powers of two where they use 0.7, plus mask_y1, two residuals without activation, ReLU
EPILOGUES = {
    "plain": Epilogue(),
    "lrelu": Epilogue(act=ACT_LRELU),
    "lrelu_r1_y0": Epilogue(act=ACT_LRELU, r1=0.5, y0=True),
    "mask": Epilogue(m=True),
    "mask_acc": Epilogue(m=True, acc=True),
    "mask_r1": Epilogue(m=True, r1=0.5),
    "generic": Epilogue(act=ACT_LRELU, alpha=0.5, y0=True, r1=0.5, r2=-0.25, acc=True, m=True, y1=True),
    "mask_y1": Epilogue(m=True, y1=True, r1=-0.25),
    "r1_r2": Epilogue(alpha=0.25, r1=-0.5, r2=1.0),
    "relu": Epilogue(act=ACT_RELU),
    "m_relu": Epilogue(m=True, m_relu=True),
}
VARIANTS = ["plain", "lrelu", "lrelu_r1_y0", "mask", "mask_acc", "mask_r1", "generic", "mask_y1", "r1_r2"]
FEW = ["lrelu", "mask_acc", "generic"]


# ================================================================================================ cases
# kind -> (kernel size, stride): "k3" 3x3 s1 p1 forward (up = 1 | 2), "s2d" 4x4 s2 p1 forward through the space-to-depth view,
# "dgrad3" / "dgrad4" the data gradients of those two (dgrad4: four parity classes through ssr_conv2d_batch), "gather" one slice of the
# gather-form dense-block backward (engine.gather_dgrad over ParamStore.add_rdb_gather: slice k <- [dpre_(k+1) .. dpre_4 | d_out])
# "k4": the 4x4 stride-2 forward where the layer is kept off the space-to-depth path (ConvSpec.s2d = False): the pipelined kernel's own form
KINDS = {"k3": (3, 1), "s2d": (4, 2), "k4": (4, 2), "dgrad3": (3, 1), "dgrad4": (4, 2), "gather": (3, 1)}
GATHER_NF, GATHER_GC, GATHER_A5 = 64, 32, 0.25           # conv5's scale is folded into the gathered table: a power of two here


@dataclass(frozen=True)
class Case:
    family: str
    mode: str
    kind: str
    B: int
    H: int                                # STORED input size
    W: int
    cin: int                              # contracted channels of the weight (Cin_w; of dy for the dgrad kinds)
    cout: int                             # output channels
    variant: str = "lrelu"
    up: int = 1
    cin_view: Optional[int] = None        # Cin of the view: a multiple of 8 >= cin; default rup(cin, 8)
    c1: int = 0                           # > 0: two input views, x of c1 channels and x2 of cin - c1
    env: Tuple[Tuple[str, str], ...] = ()

    @property
    def name(self):
        tag = f"{self.family}-{self.mode}-{self.kind}-{self.B}x{self.H}x{self.W}-{self.cin}to{self.cout}-{self.variant}"
        tag += f"-up{self.up}" if self.up > 1 else ""
        tag += f"-view{self.cin_view}" if self.cin_view else ""
        tag += f"-x2at{self.c1}" if self.c1 else ""
        return tag + "".join(f"-{k[4:]}{v}" for k, v in self.env)

    @property
    def view(self):
        return self.cin_view or rup(self.cin, 8)

    @property
    def out_hw(self):
        if self.kind in ("s2d", "k4"):
            return self.H // 2, self.W // 2
        if self.kind == "dgrad4":
            return 2 * self.H, 2 * self.W
        return self.H * self.up, self.W * self.up

    @property
    def K(self):
        k = KINDS[self.kind][0]
        return self.cin * (4 if self.kind == "dgrad4" else k * k)       # (a parity class sees 2 x 2 of the 4 x 4 taps)

    @property
    def ep(self):
        return EPILOGUES[self.variant]

    @property
    def bias(self):
        return self.kind in ("k3", "s2d", "k4")

    def data_key(self):
        """what the data depends on: not the family, the switches or the batch (image n of a case is image n of every batch)"""
        return (self.kind, self.H, self.W, self.cin, self.cout, self.up, self.view, self.c1, arithmetic(self.family, self.mode)[0],
                integer_x(self.family, self.mode))


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def weight_shape(case):
    k = KINDS[case.kind][0]
    return (case.cout, case.cin, k, k) if case.bias else (case.cin, case.cout, k, k)


MAX_B = 3


@lru_cache(maxsize=None)
def _data(key, B):
    kind, H, W, cin, cout, up, view, c1, lattice, xint = key
    case = Case("x3r", "fp32", kind, B, H, W, cin, cout, up=up, cin_view=view, c1=c1)
    Ho, Wo = case.out_hw
    lat = LATTICES[lattice]
    nb = max(B, MAX_B)                        # image n is the same at every batch size up to MAX_B
    x = lat((nb, H, W, view), _seed(key, "x"))[:B].clone()
    if xint:
        x = x.round()
    x[..., cin:] = 0.0                        # the channels of the view that the weight does not have
    w = lat(weight_shape(case), _seed(key, "w"))
    share = keep_share(lattice, case.K)
    if share < 1.0:
        gen = torch.Generator().manual_seed(_seed(key, "keep"))
        w = w * (torch.rand(w.shape, generator=gen) < share)
    out = {"x": x, "w": w, "bias": coarse_lattice((cout,), _seed(key, "bias"))}
    for name in ("r1", "r2", "yold", "m"):
        out[name] = coarse_lattice((nb, Ho, Wo, cout), _seed(key, name))[:B].clone()
    gen = torch.Generator().manual_seed(_seed(key, "mzero"))
    out["m"][torch.rand((nb, Ho, Wo, cout), generator=gen)[:B] < 0.25] = 0.0          # exact zeros: the 0.2 side
    return out


def inputs(case):
    """name -> fp32 CPU tensor, NHWC (shared between tests: do not modify): x [B, H, W, view] with zeros past cin, w in the reference's
    layout, bias, and r1 / r2 / yold / m [B, Ho, Wo, cout]"""
    return _data(case.data_key(), case.B)


# ================================================================================================ float64 reference
def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def contract(x, w, kind, up=1):
    """x [B, C, H, W], w in the reference's layout, float64 -> [B, Cout, Ho, Wo]: what the descriptor contract prescribes"""
    if kind == "k3":
        if up == 2:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        return F.conv2d(x, w, padding=1)
    if kind in ("s2d", "k4"):
        return F.conv2d(x, w, stride=2, padding=1)
    if kind in ("dgrad3", "gather"):
        return F.conv_transpose2d(x, w, padding=1)
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def term_pairs(x, w, pieces):
    """the (x, w) operand pairs whose convolutions add up to the mode's result"""
    if pieces is None:
        return [(x, w)]
    if pieces == "bf16":
        (xh, xl), (wh, wl) = split_planes(x.float()), split_planes(w.float())
    else:
        (xh, xl), (wh, wl) = half_planes(x.float()), half_planes(w.float(), WSHIFT)
    return [(xh.double(), wh.double()), (xh.double(), wl.double()), (xl.double(), wh.double())]


def accumulate(case, data, conv=contract):
    """-> (acc + bias, sum |terms| + |bias|) float64 [B, Cout, Ho, Wo]"""
    x, w = _nchw(data["x"][..., :case.cin]), data["w"].double()
    acc = mag = 0.0
    for xx, ww in term_pairs(x, w, arithmetic(case.family, case.mode)[1]):
        acc = acc + conv(xx, ww, case.kind, case.up)
        mag = mag + conv(xx.abs(), ww.abs(), case.kind, case.up)
    if case.bias:
        b = data["bias"].double().view(1, -1, 1, 1)
        acc, mag = acc + b, mag + b.abs()
    return acc, mag


def ordered_partitions(items):
    """every way to deal `items` into a sequence of non-empty groups: 1, 1, 3, 13 for 0..3 items"""
    items = list(items)
    if not items:
        return [[]]
    out = []
    for p in ordered_partitions(items[1:]):
        for i in range(len(p)):
            out.append(p[:i] + [[items[0]] + p[i]] + p[i + 1:])
        for i in range(len(p) + 1):
            out.append(p[:i] + [[items[0]]] + p[i:])
    return out


def r32(t):
    """one fp32 rounding of a float64 tensor"""
    return t.float().double()


def finish(pre, ep, data, bf16=False):
    """the epilogue on the exact pre-activation `pre` [B, C, Ho, Wo] float64 -> {"y", "y0", "y1"}: stacks [n, B, Ho, Wo, C] fp32 of the
    fp32 evaluations an element may equal (n = the ordered partitions of the terms that follow s0), as stored (bf16: rounded once more)"""
    if ep.act == ACT_LRELU:
        v = torch.where(pre > 0, pre, r32(pre * SLOPE))          # (pre * SLOPE is exact in float64: 24 x 24 bits)
    elif ep.act == ACT_RELU:
        v = pre.clamp(min=0.0)
    else:
        v = pre
    s0 = ep.alpha * v                                            # a power of two: exact
    assert torch.equal(r32(s0), s0), "alpha s0 is no fp32 number"
    terms = {}
    if ep.r1 is not None:
        terms["r1"] = ep.r1 * _nchw(data["r1"])
    if ep.r2 is not None:
        terms["r2"] = ep.r2 * _nchw(data["r2"])
    if ep.acc:
        terms["yold"] = _nchw(data["yold"])
    s1s = []
    for part in ordered_partitions(terms):
        a = s0
        for block in part:
            a = r32(a + sum(terms[k] for k in block))            # (each float64 sum is exact: operands within 2^-40 .. 2^12)
        s1s.append(a)
    if ep.m:
        m = _nchw(data["m"])
        fac = torch.where(m > 0, torch.ones_like(m), torch.full_like(m, 0.0 if ep.m_relu else SLOPE))
        ys = [r32(s * fac) for s in s1s]
    else:
        ys = s1s

    def stored(ts):
        t = torch.stack(ts).float().permute(0, 1, 3, 4, 2).contiguous()
        return t.bfloat16().float() if bf16 else t
    return {"y": stored(ys), "y0": stored([s0]), "y1": stored(s1s)}


def rounded_elements(pre, ep, data):
    """where a rounding lies on the path of y1 / of y: [B, C, Ho, Wo] bool each"""
    r1 = (pre < 0) if ep.act == ACT_LRELU else torch.zeros_like(pre, dtype=torch.bool)
    ry = r1 | ((_nchw(data["m"]) <= 0) & (not ep.m_relu)) if ep.m else r1
    return r1, ry


def expected(case, data=None):
    """-> ({"y", "y0", "y1"} candidate stacks [n, B, Ho, Wo, C] fp32, margin).  Asserts the exactness condition for every output element
    and, where no rounding lies on an element's path, that all candidates are the float64 value."""
    if data is None:
        return _expected(case)
    return _expected_of(case, data)


@lru_cache(maxsize=None)
def _expected(case):
    return _expected_of(case, inputs(case))


def _expected_of(case, data):
    lattice = arithmetic(case.family, case.mode)[0]
    pre, mag = accumulate(case, data)
    margin = float(mag.max()) * 2.0 ** data.get("granule_bits", GRANULE_BITS[lattice]) / 2.0 ** 24
    assert margin < 1.0, f"{case.name}: sum |terms| is {margin:.3f} of 2^24 granules: the sum is not exact in every order"
    assert torch.equal(r32(pre), pre), f"{case.name}: the pre-activation is no fp32 number"
    ep = case.ep
    out = finish(pre, ep, data, bf16=case.mode == "bf16")
    full = finish(pre, ep, data)
    r1, ry = rounded_elements(pre, ep, data)
    for name, rounded in (("y1", r1), ("y", ry)):
        same = (full[name] == full[name][:1]).all(0).permute(0, 3, 1, 2)
        assert bool(same[~rounded].all()), f"{case.name} {name}: an element without a rounding on its path has more than one target"
    # the exact path once more without any rounding: the float64 value itself is the target
    s1 = ep.alpha * (pre if ep.act != ACT_RELU else pre.clamp(min=0.0))
    for key, beta in (("r1", ep.r1), ("r2", ep.r2), ("yold", 1.0 if ep.acc else None)):
        if beta is not None:
            s1 = s1 + beta * _nchw(data[key])
    assert torch.equal(full["y1"][0].permute(0, 3, 1, 2).double()[~r1], s1[~r1]), f"{case.name}: y1 is not the float64 value"
    return out, margin


def member(got, cands):
    """[B, Ho, Wo, C] bool: the element equals one of its candidates (NaN equals nothing)"""
    return (got.unsqueeze(0) == cands).any(0)


def margin_line(case):
    _, m = expected(case)
    return f"{case.name}: K = {case.K}, sum |terms| = {m:.4f} of 2^24 granules"


# ================================================================================================ the shared case lists
def _cases(family, modes, kind, grids, Bs, chans, variants, **kw):
    return [Case(family, mode, kind, B, h, w, ci, co, v, **kw) for mode in modes for (h, w) in grids for B in Bs for (ci, co) in chans
            for v in variants]


def _unique(cases):
    return list(dict.fromkeys(cases))


# against 8 x 16-pixel tiles, and the 4 x 16 of x3r's TH = 4, of the K-resident kernel and of the pipelined kernel's small launches
SMALL_GRIDS = [(1, 1), (2, 3), (4, 16), (5, 17), (8, 16), (9, 17), (7, 15), (16, 33)]
BIG_GRIDS = [(1, 1), (31, 15), (32, 16), (33, 17), (24, 40)]                  # against 32 x 16-pixel tiles
THIN_GRIDS = [(1, 1), (2, 3), (8, 32), (9, 33), (7, 31), (17, 17)]                # against the 8 x 32-pixel tiles of the thin kernel
MID = (9, 17)
CINS = [8, 16, 24, 40, 72, 128, 144, 192, 272]           # 1, 1, 2, 3, 5, 8, 9, 12, 17 chunks of 16; 8, 24, 40, 72: Cin % 16 == 8
TWO_VIEWS = [(96, 64, 32), (32, 64, 32), (128, 64, 64), (16, 64, 32)]         # tests/test_gpu_conv_x3.py::test_ring_x3_conv_two_input_views
MODES_OF = {"x3r": ["fp32x3", "fp32", "fp32h"], "x3q": ["fp32x3"], "pipelined": ["bf16", "fp32", "fp32x3", "fp32h"], "res": ["bf16", "fp32"],
            "thin": ["bf16", "fp32", "fp32x3", "fp32h"], "bigx3": ["fp32x3", "fp32h"], "big": ["bf16"], "ws": ["bf16"]}


def small_tile_cases(family):
    """x3r, x3q, res, pipelined: 3x3 stride 1 on 8 x 16-pixel tiles"""
    modes = MODES_OF[family]
    cins = [c for c in CINS if not (family == "res" and c > 192)]            # (272 channels do not fit the K-resident kernel's LDS)
    out = _cases(family, modes, "k3", SMALL_GRIDS, (1, 3), [(64, 32)], ["lrelu"])
    out += _cases(family, modes, "k3", [MID], (1,), [(c, 32) for c in cins if c != 192], ["lrelu"])
    out += _cases(family, modes, "k3", [MID], (1,), [(192, 64), (72, 32)], FEW)                       # K = 1728: the largest of the model
    out += _cases(family, modes, "k3", [MID], (1,), [(3, 32), (5, 32)], ["lrelu"], cin_view=8)         # Cin_w < Cin
    out += _cases(family, modes, "k3", [MID], (1,), [(64, 64), (64, 96), (64, 128), (64, 40)], ["lrelu"])
    out += _cases(family, modes, "k3", [MID], (1,), [(96, 32)], VARIANTS)
    out += _cases(family, modes, "k3", [(4, 16)], (1,), [(64, 32)], ["plain", "mask", "generic"])       # (x3r: TH = 8 with every epilogue)
    if family == "pipelined":                                                 # its own 4x4 stride-2 form (16 / 8 channels per chunk)
        out += _cases(family, ["bf16", "fp32"], "k4", [(2, 2), (16, 32), (18, 34), (14, 30)], (1, 3), [(32, 64)], ["lrelu"])
        out += _cases(family, ["bf16", "fp32"], "k4", [(18, 34)], (1,), [(24, 40), (8, 32), (72, 32)], FEW)
    if family != "res":                                                       # (ReLU epilogues outside the split modes: the pipelined kernel)
        relu_modes = [m for m in modes if m in ("fp32x3", "fp32h") or family == "pipelined"]
        out += _cases(family, relu_modes, "k3", [MID], (1,), [(96, 32)], ["relu", "m_relu"])
    for c1, c2, co in TWO_VIEWS:
        out += _cases(family, modes, "k3", [MID], (2,), [(c1 + c2, co)], ["mask"], c1=c1)
    if family in ("x3r", "pipelined"):
        dmodes = [m for m in modes if m != "fp32h"]                           # (the backward of mode fp32h is fp32x3's)
        out += _cases(family, dmodes, "dgrad3", [MID], (1,), [(32, 64), (40, 24)], ["mask_r1"])
    if family != "res":
        # slices 4, 2 and 1 of a dense block's backward: d_out alone; two and three earlier slices in front of it (x2 at channel 64, 96)
        gmodes = [m for m in modes if m != "fp32h"]
        for c1 in (0, 64, 96):
            out += _cases(family, gmodes, "gather", [MID], (2,), [(c1 + GATHER_NF, GATHER_GC)], ["mask"], c1=c1)
    return [c for c in out if family != "res" or res_fits(c)]


def res_fits(case):
    """res_shape_ok (csrc/conv_res.hip:214-222): the whole contraction in LDS, (112 + 9 x 32) rows of 64 bytes per chunk of 16 (fp32) or
    32 (bf16) channels within 160 KB: six chunks.  The family cannot be forced - a layer it refuses goes on to the pipelined kernel
    without a word - so its list holds only what fits (and at most 2048 tile x channel-group items: every case here)."""
    ck = 16 if case.mode == "fp32" else 32
    return -(-case.view // ck) * (112 + 9 * 32) * 64 <= 160 * 1024


def form_cases():
    """the launch size alone selects x3r's TH = 8 and its <2, 1> form (xr_tile_height, xr_wide_form of csrc/conv_x3r.hip: more than 160
    workgroups) and the 8 x 16 tile of the pipelined kernel outside the split modes (pick_tile of csrc/conv.hip: 384 tiles and up): one
    case per arithmetic and form at B = 32, 32 x 32"""
    return _cases("x3r", MODES_OF["x3r"], "k3", [(32, 32)], (32,), [(64, 32), (64, 64)], ["lrelu"]) + \
        _cases("x3r", ["fp32x3"], "k3", [(32, 32)], (32,), [(64, 32)], ["plain"]) + \
        _cases("pipelined", ["bf16", "fp32"], "k3", [(32, 32)], (32,), [(64, 96)], ["lrelu"])


def big_tile_cases(family):
    """big (bf16), bigx3 / bigh3: 32 x 16-pixel x 64-channel tiles, persistent over images under both settings of SSR_CONV_BIG_G"""
    modes = MODES_OF[family]
    out = []
    for g in ("1", "2"):
        env = (("SSR_CONV_BIG_G", g),)
        out += _cases(family, modes, "k3", BIG_GRIDS, (1, 3), [(64, 64)], ["lrelu"], env=env)
        out += _cases(family, modes, "k3", [(33, 17)], (3,), [(192, 64), (72, 64)], FEW, env=env)
        smodes = [m for m in modes if m != "bf16"] if family == "bigx3" else modes
        out += _cases(family, smodes, "s2d", [(16, 16), (34, 66)], (1, 3), [(32, 64), (64, 64)], ["lrelu"], env=env)
    cins = [c for c in CINS if c != 192 and not (family == "big" and c < 32)]
    out += _cases(family, modes, "k3", [MID], (1,), [(c, 64) for c in cins], ["lrelu"])
    if family == "bigx3":
        out += _cases(family, modes, "k3", [MID], (1,), [(3, 64), (5, 64)], ["lrelu"], cin_view=8)
    out += _cases(family, modes, "k3", [MID], (1,), [(64, 128), (64, 40)], ["lrelu"])
    out += _cases(family, modes, "k3", [MID], (1,), [(96, 64)], VARIANTS)
    out += _cases(family, modes, "k3", [(8, 8), (9, 7)], (2,), [(64, 64)], FEW, up=2)
    return out


def parity_class_cases():
    """the four parity classes of a 4x4 stride-2 dgrad through ssr_conv2d_batch: on the big-tile kernel (SSR_X3_BIGTILE2 = 2, KT = 2) under
    both group settings, and as the library deals them by itself at this size (bf16: one pipelined launch; fp32x3: four)"""
    out = []
    for g in ("1", "2"):
        env = (("SSR_CONV_BIG_G", g), ("SSR_X3_BIGTILE2", "2"))
        out += _cases("bigx3", ["fp32x3"], "dgrad4", [(16, 16), (10, 12)], (1, 3), [(64, 64), (72, 64)], ["mask_r1"], env=env)
    out += _cases("pipelined", ["fp32x3", "bf16", "fp32"], "dgrad4", [(16, 16), (10, 12)], (1, 3), [(64, 64)], ["mask_r1"])
    for g in ("1", "2"):                                                      # bf16: conv_big_kernel4 (SSR_CONV_BIGTILE2 = 2)
        env = (("SSR_CONV_BIG_G", g), ("SSR_CONV_BIGTILE2", "2"))
        out += _cases("big", ["bf16"], "dgrad4", [(16, 16), (10, 12)], (1, 3), [(64, 64), (72, 64)], ["mask_r1"], env=env)
    return out


def ws_cases():
    out = _cases("ws", ["bf16"], "k3", SMALL_GRIDS, (1, 3), [(64, 64)], ["lrelu"])                      # (WS_TH x WS_TW = 8 x 16)
    out += _cases("ws", ["bf16"], "k3", [MID], (1,), [(8, 32), (16, 32), (24, 32), (40, 64), (64, 40), (32, 96)], FEW)
    out += _cases("ws", ["bf16"], "k3", [MID], (1,), [(3, 32)], ["lrelu"], cin_view=8)
    out += _cases("ws", ["bf16"], "k3", [MID], (1,), [(64, 64)], VARIANTS)
    out += _cases("ws", ["bf16"], "k3", [(8, 8), (9, 7)], (2,), [(64, 64)], FEW, up=2)
    return out


def thin_cases():
    modes = MODES_OF["thin"]
    out = _cases("thin", modes, "k3", THIN_GRIDS, (1, 3), [(64, 3)], ["lrelu"])
    out += _cases("thin", modes, "k3", [MID], (1,), [(8, 1), (24, 5), (40, 8), (64, 1), (16, 3)], FEW)
    out += _cases("thin", modes, "k3", [MID], (1,), [(3, 3), (5, 8)], ["lrelu"], cin_view=8)
    out += _cases("thin", modes, "k3", [MID], (1,), [(48, 3)], VARIANTS)
    return out


GPU_CASES = {
    "x3r": small_tile_cases("x3r"), "forms": form_cases(), "x3q": small_tile_cases("x3q"), "pipelined": small_tile_cases("pipelined"),
    "res": small_tile_cases("res"), "thin": thin_cases(), "bigx3": big_tile_cases("bigx3"), "big": big_tile_cases("big"), "ws": ws_cases(),
    "parity-classes": parity_class_cases(),
}
GPU_CASES = {k: _unique(v) for k, v in GPU_CASES.items()}
# the fp16 specifics (tests/test_gpu_conv_exact.py builds their data itself)
F16_SINGLE = [Case(f, "fp32h", "k3", 1, 1, 1, 16, 32 if f != "bigx3" else 64, "plain") for f in ("x3r", "bigx3", "pipelined")]
F16_SUBNORMAL = [Case(f, "fp32h", "k3", 1, 5, 7, 16, 32 if f != "bigx3" else 64, "plain") for f in ("x3r", "bigx3", "pipelined")]
ALL_CASES = [c for cs in GPU_CASES.values() for c in cs]


def single_product_data(case):
    """one chunk, a 1 x 1 grid (only the centre tap meets data) and ONE non-zero channel: every output is one product of three terms"""
    d = {k: v.clone() for k, v in inputs(case).items()}
    d["x"][..., 1:] = 0.0
    d["bias"].zero_()
    return d


def subnormal_lo_data(case):
    """x = +-1 + b 2^-16 (lo = b 2^-16 is an fp16 subnormal), |w| = 1 + b 2^-12: the terms are multiples of 2^-16 x 1 = 2^-16 and
    1 x 2^-12; K = 144, sum |terms| < 145 << 2^24 x 2^-16 = 256"""
    d = {k: v.clone() for k, v in inputs(case).items()}
    for key in ("x", "w"):
        gen = torch.Generator().manual_seed(_seed(case.name, key, "sub"))
        shape = d[key].shape
        sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
        b = torch.randint(-1, 2, shape, generator=gen).double()
        d[key] = (sign * (1.0 + b * 2.0 ** (-16 if key == "x" else -12))).float()
    d["x"][..., case.cin:] = 0.0
    d["granule_bits"] = 16
    return d


# ================================================================================================ the runner
@contextlib.contextmanager
def environ(values):
    old = {k: os.environ.get(k) for k in values}
    try:
        os.environ.update(values)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SENT_BITS = {4: 0x4B8E4D2B, 2: 0x4B8E}           # a finite value no lattice sum takes (about 1.9e7), the same in fp32 and bf16 bits


class Sliced:
    """values [B, H, W, c] as the channels [coff, coff + c) of a buffer of coff + rup(c, 8) + X_GUARD channels with one pixel row of margin
    above and below, everything but the view filled with `fill` (a float, or None: the sentinel bit pattern)"""

    def __init__(self, values, dtype, coff=X_GUARD, fill=None, tail=X_GUARD):
        B, H, W, c = values.shape
        self.c, self.coff, self.cs = c, coff, coff + rup(c, 8) + tail
        self.row = W * self.cs
        n = B * H * W * self.cs
        self.flat = torch.empty(n + 2 * self.row, dtype=dtype, device="cuda")
        ibits = self.flat.view(torch.int32 if dtype == torch.float32 else torch.int16)
        if fill is None:
            ibits.fill_(SENT_BITS[self.flat.element_size()])
        else:
            self.flat.fill_(fill)
        self.t = self.flat[self.row:self.row + n].view(B, H, W, self.cs)
        self.inside = torch.zeros_like(self.flat, dtype=torch.bool)
        self.inside[self.row:self.row + n].view(B, H, W, self.cs)[..., coff:coff + c] = True

    def set(self, values):
        self.t[..., self.coff:self.coff + self.c] = values.to(self.flat.dtype).cuda()
        self.before = self.flat.clone()
        return self

    def bits(self, t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def outside_unchanged(self):
        return bool((self.bits(self.flat)[~self.inside] == self.bits(self.before)[~self.inside]).all())

    def unchanged(self):
        return torch.equal(self.bits(self.flat), self.bits(self.before))

    def read(self):
        return self.t[..., self.coff:self.coff + self.c].float().cpu()


def _apply_epilogue(d, ep, hip, cout, bufs):
    d.act, d.alpha = ep.act, ep.alpha
    if ep.y0:
        d.y0 = hip.view(bufs["y0"].t, bufs["y0"].coff)
    if ep.y1:
        d.y1 = hip.view(bufs["y1"].t, bufs["y1"].coff)
    if ep.r1 is not None:
        d.r1, d.r1_nc, d.beta1 = hip.view(bufs["r1"].t, bufs["r1"].coff), cout, ep.r1
    if ep.r2 is not None:
        d.r2, d.r2_nc, d.beta2 = hip.view(bufs["r2"].t, bufs["r2"].coff), cout, ep.r2
    if ep.m:
        d.m, d.m_c0, d.m_c1, d.m_relu = hip.view(bufs["m"].t, bufs["m"].coff), 0, cout, 1 if ep.m_relu else 0
    d.accumulate = 1 if ep.acc else 0


def run(case, data=None):
    """One case through engine.ParamStore / pack(), engine._ConvBuilder.conv or .dgrad and ssr_conv2d_impl with the family forced (the
    four parity classes of "dgrad4": ssr_conv2d_batch).  Every view is a channel slice: x (and x2) at channel 8 of a buffer whose other
    channels and margin rows hold X_SENTINEL (NaN); y, y0, y1 at channel 8 of buffers that hold a sentinel bit pattern everywhere
    else (and in the view itself unless the case accumulates); r1, r2, m at channel 0 with NaN behind their `cout` channels.
    -> y, y0, y1 [B, Ho, Wo, cout] fp32 CPU (None where the case has none), symbol (ssr_conv2d_symbol_impl: the kernel that launch
    started.  "dgrad4" goes through ssr_conv2d_batch, which takes no impl and reports nothing: there the symbol is ssr_conv2d_symbol of
    one class where the library deals the classes itself, and select's answer for the family where a switch forces the big tile - it
    does not show which path the batch took), guards_ok, inputs_ok"""
    from satlas_super_resolution_amd import engine, hip
    data = inputs(case) if data is None else data
    ep, mode = case.ep, case.mode
    dt = hip.dtype_code(mode)
    tdt = torch.bfloat16 if mode == "bf16" else torch.float32
    k, stride = KINDS[case.kind]
    fwd = case.bias
    with environ(dict(case.env)):
        if case.kind == "gather":
            st, gk = _gather_store(case, data, dt, engine)
        else:
            spec = engine.ConvSpec("c", case.cout, case.cin, k, stride, True, False, s2d=None if case.kind == "s2d" else False) if fwd else \
                engine.ConvSpec("c", case.cin, case.cout, k, stride, False, False)
            st = engine.ParamStore([spec], dt)
            sd = {"c.weight": data["w"]}
            if fwd:
                sd["c.bias"] = data["bias"]
            st.load_state_dict(sd)
        st.pack()
        sent = X_SENTINEL
        c1 = case.c1 or case.view
        xs = [Sliced(data["x"][..., :c1], tdt, fill=sent).set(data["x"][..., :c1])]
        if case.c1:
            xs.append(Sliced(data["x"][..., c1:], tdt, fill=sent).set(data["x"][..., c1:]))
        Ho, Wo = case.out_hw
        blank = torch.empty(case.B, Ho, Wo, case.cout)
        bufs = {}
        for name in ("r1", "r2", "m"):
            bufs[name] = Sliced(data[name], tdt, coff=0, fill=float("nan"), tail=0).set(data[name])
        for name in ("y", "y0", "y1"):
            bufs[name] = Sliced(blank, tdt)
            bufs[name].before = bufs[name].flat.clone()
        if ep.acc:
            bufs["y"].set(data["yold"])
        cb, L = engine._ConvBuilder(st, case.B), engine.Launcher()
        xv, yv = hip.view(xs[0].t, xs[0].coff), hip.view(bufs["y"].t, bufs["y"].coff)
        if fwd:
            assert bool(st.s2d["c"]) == (case.kind == "s2d"), "the space-to-depth path is what the kind names"
            descs = [cb.conv(L, "c", xv, case.H, case.W, yv, up=case.up, cin=c1)]
        elif case.kind == "gather":
            x1v, x2v = (xv, hip.view(xs[1].t, xs[1].coff)) if case.c1 else (hip.NULL_VIEW, xv)
            descs = [engine.gather_dgrad(cb, L, "b", gk, x1v, case.c1, x2v, GATHER_NF, case.H, case.W, yv, case.cout)]
            assert (descs[0].Cin, descs[0].Cin2) == ((case.c1, GATHER_NF) if case.c1 else (GATHER_NF, 0))
        else:
            cb.dgrad(L, "c", xv, case.H, case.W, yv, cin_dy=c1)
            descs = [cb.keep[-1]] if stride == 1 else list(L.calls[0][1][0])
        for d in descs:
            if case.c1 and case.kind != "gather":
                d.x2, d.Cin2 = hip.view(xs[1].t, xs[1].coff), case.view - c1
            _apply_epilogue(d, ep, hip, case.cout, bufs)
        lib = hip.lib()
        if case.kind == "dgrad4":
            arr = cb.array(descs)
            hip.check(lib.ssr_conv2d_batch(arr, len(descs), hip.stream_ptr()), f"ssr_conv2d_batch {case.name}")
        else:
            hip.check(lib.ssr_conv2d_impl(C.byref(descs[0]), hip.stream_ptr(), IMPL[case.family]), f"impl {IMPL[case.family]} {case.name}")
        # ssr_conv2d_batch takes no impl: where the library deals the classes by itself the symbol is that of ssr_conv2d for one class; where
        # a switch sends the batch to a big-tile kernel it is what select answers for that family - that the family CAN run the class, not
        # a record of which path the batch took (the library has no report for a batch)
        batch_auto = case.kind == "dgrad4" and case.family == "pipelined"
        symbol = hip.conv_symbol(descs[0], 0 if batch_auto else IMPL[case.family])
        torch.cuda.synchronize()
    outs = {name: bufs[name].read() if (name == "y" or getattr(ep, name)) else None for name in ("y", "y0", "y1")}
    return SimpleNamespace(
        **outs, symbol=symbol,
        guards_ok=all(bufs[n].outside_unchanged() for n in ("y", "y0", "y1")) and all(bufs[n].unchanged() for n in ("y0", "y1") if not getattr(ep, n)),
        inputs_ok=all(b.unchanged() for b in xs + [bufs[n] for n in ("r1", "r2", "m")]))


def _gather_store(case, data, dt, engine):
    """the five convs of a dense block whose gathered table of slice k holds data["w"]: rows [W_(k+1) .. W_4 | a5 W_5][:, slice k] of the
    later convs' weights (everything else in them: other lattice values, which the slice must not see)"""
    nf, gc = GATHER_NF, GATHER_GC
    gk = 4 - case.c1 // gc
    assert case.cout == gc and case.cin == case.c1 + nf and case.c1 % gc == 0 and 1 <= gk <= 4
    names = [f"b.conv{j}" for j in range(1, 6)]
    st = engine.ParamStore([engine.ConvSpec(names[j - 1], gc if j < 5 else nf, nf + (j - 1) * gc, 3, 1, True, False, dgrad_packed=False)
                            for j in range(1, 6)], dt)
    lo, row, sd = nf + (gk - 1) * gc, 0, {}
    for j in range(1, 6):
        co = gc if j < 5 else nf
        w = coarse_lattice((co, nf + (j - 1) * gc, 3, 3), _seed(case.name, "distractor", j))
        if j > gk:
            w[:, lo:lo + gc] = data["w"][row:row + co] / (GATHER_A5 if j == 5 else 1.0)
            row += co
        sd[names[j - 1] + ".weight"], sd[names[j - 1] + ".bias"] = w, torch.zeros(co)
    assert row == case.cin
    st.load_state_dict(sd)
    st.add_rdb_gather("b", nf, gc, GATHER_A5)
    return st, gk


def mismatch(case, res, data=None):
    """None, or what differs: per output the number of elements outside their candidates, the first one and the difference in granules"""
    exp, margin = expected(case, data)
    g = (data or {}).get("granule_bits", GRANULE_BITS[arithmetic(case.family, case.mode)[0]])
    msgs = []
    for name in ("y", "y0", "y1"):
        got = getattr(res, name)
        if got is None:
            continue
        ok = member(got, exp[name])
        if not bool(ok.all()):
            first = tuple(int(v) for v in (~ok).nonzero()[0])
            want = exp[name][(slice(None),) + first]
            diff = float(torch.nan_to_num((got - exp[name][0]).abs(), nan=float("inf"))[~ok].max()) * 2 ** g
            msgs.append(f"{name}: {int((~ok).sum())} of {ok.numel()} elements differ, first at {first}: got {float(got[first])!r}, want one of "
                        f"{sorted(set(want.tolist()))}; largest difference {diff:g} granules (margin {margin:.3f})")
    if not res.guards_ok:
        msgs.append("a write outside the views of y / y0 / y1")
    if not res.inputs_ok:
        msgs.append("an input buffer was written")
    return f"{case.name} [{res.symbol}]: " + "; ".join(msgs) if msgs else None
