"""SRCNN and HighResNet on MI355X: the two WorldStrat baselines the reference trains with `model_type: L2Model` - same registry
names, constructor arguments, forward contract and state_dict layout as ssr/archs/srcnn_arch.py:12-195 and highresnet_arch.py:9-77.

    forward(x: float32[B, revisits, C, H, W]) -> float32[B, 1, out_channels, zoom H, zoom W]

The work is done by L2Plan through libssr_hip.so: the reflect-padded 3 x 3 convolutions run as pad-0 ssr_conv2d launches over
(H+2) x (W+2) buffers, everything between them (PReLU with its learned slope, Dropout, residual adds, the padding itself, the
revisit -> channel views, the PixelShuffle tail) in the kernels of csrc/l2net.hip.  Exact fp32 only.  No CPU path: the CPU
statement of both networks is l2_reference.py.

state_dict (pinned by tests/golden/l2_*_tiny.pt): the keys, shapes and order of the reference.  SRCNN lists `doubleconv2d.*` and
`residualblocks.*` again as `fusion.0.*` / `fusion.1.*` (the same tensors); HighResNet keeps those two groups as parameters its
forward never uses (no gradient; the optimizer never touches them, as torch leaves `grad is None` alone) and lists its one shared
FusionBlock ceil(log2(revisits)) times; both carry the six tensors of a zero-channel mask encoder, stored and loaded, never used.

What is accepted: mask_channels 0 and no `mask` argument, use_reference_frame False, kernel_size 3, sr_kernel_size 1, hidden_channels
divisible by zoom_factor^2, residual_layers >= 0, revisits >= 1; anything else raises NotImplementedError naming the key.
`output_size` must be the network's natural output - an int equal to zoom*H with H == W, or a pair (zoom*H, zoom*W): kornia's
Resize returns its input unchanged when the size already matches [recalled]; a real resample raises NotImplementedError naming
`output_size` (checked at the first forward, when H and W are known; HighResNet's forward never resizes, highresnet_arch.py:69-77).

Dropout: eval() makes it the identity.  train() drops with p = 0.5 and scales by 2 after each PReLU of every DoubleConv2d, from the
generator of ssr_dropout_mask (Philox4x32-10 keyed by `manual_seed`, counted by a device step counter and the site index; DESIGN.md
section 4) - torch's own random stream is not reproduced.  `dropout_masks=` (bool tensors, one per site in forward order, NCHW) replaces
the generator: the hook the parity tests use.
"""
from __future__ import annotations

import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .. import engine, hip
from ..engine import ConvSpec, Launcher, WgradBatch, conv_desc, rup, wgrad_args
from ..hip import PackItem, PreluReflectDesc, SrTailDesc, View, view
from ..l2_reference import mask_words, pack_mask_nhwc
from ..registry import ARCH_REGISTRY
from .hipnet import ConvParams


# ------------------------------------------------------------------------------------------------ options
def check_compute_dtype(compute_dtype):
    if compute_dtype not in ("fp32", "float32"):
        raise NotImplementedError(f"compute_dtype={compute_dtype!r}: SRCNN / HighResNet run in exact fp32 only (the split modes' LeakyReLU "
                                  "decision fix-up has no PReLU counterpart)")


def check_arch_options(kw: Dict):
    """the constructor arguments this path cannot honour, by name, before any launch"""
    if int(kw["mask_channels"]) != 0:
        raise NotImplementedError(f"mask_channels={kw['mask_channels']!r}: only 0 (no mask encoder input)")
    if kw.get("use_reference_frame", False):
        raise NotImplementedError("use_reference_frame: only False")
    if int(kw["kernel_size"]) != 3:
        raise NotImplementedError(f"kernel_size={kw['kernel_size']!r}: only 3")
    if int(kw["sr_kernel_size"]) != 1:
        raise NotImplementedError(f"sr_kernel_size={kw['sr_kernel_size']!r}: only 1")
    z, h = int(kw["zoom_factor"]), int(kw["hidden_channels"])
    if z < 1 or h < 1 or h % (z * z):
        raise NotImplementedError(f"hidden_channels={h!r}: must be divisible by zoom_factor^2 = {z * z}")
    if h % 8:
        raise NotImplementedError(f"hidden_channels={h!r}: the NHWC channel slices are multiples of 8")
    if h // (z * z) > 32 or int(kw["out_channels"]) > 8:
        raise NotImplementedError(f"hidden_channels={h!r} / out_channels={kw['out_channels']!r}: the tail kernel takes up to 32 channels "
                                  "behind the shuffle and 8 outputs")
    if int(kw["residual_layers"]) < 0:
        raise NotImplementedError(f"residual_layers={kw['residual_layers']!r}: must be >= 0")
    if int(kw["revisits"]) < 1:
        raise NotImplementedError(f"revisits={kw['revisits']!r}: must be >= 1")
    osz = kw["output_size"]
    if not (isinstance(osz, int) or (isinstance(osz, (tuple, list)) and len(osz) == 2 and all(isinstance(v, int) for v in osz))):
        raise NotImplementedError(f"output_size={osz!r}: an int or a pair of ints")


def check_output_size(output_size, zoom: int, H: int, W: int):
    want = (zoom * H, zoom * W)
    ok = (output_size == want[0] and H == W) if isinstance(output_size, int) else tuple(output_size) == want
    if not ok:
        raise NotImplementedError(f"output_size={output_size!r} for a {H} x {W} input: the network's natural output is {want}; a real "
                                  "resample is outside this path")


# ------------------------------------------------------------------------------------------------ parameter holders
class _Slope(nn.Module):
    """nn.PReLU()'s single learned slope (init 0.25)"""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(torch.full((1,), 0.25))


class _EmptyConv(nn.Module):
    """the mask encoder's first convolution over ZERO input channels: stored and loaded, never used"""

    def __init__(self, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, 0, 3, 3))
        self.bias = nn.Parameter(torch.zeros(cout))


def _conv(cout, cin, k=3) -> nn.Module:
    return _EmptyConv(cout) if cin == 0 else ConvParams(engine.ConvSpec("", cout, cin, k), "default")


def _double_conv(cin, cout) -> nn.Module:
    m, seq = nn.Module(), nn.Module()
    for idx, leaf in (("0", _conv(cout, cin)), ("2", _Slope()), ("4", _conv(cout, cout)), ("6", _Slope())):
        seq.add_module(idx, leaf)
    m.add_module("doubleconv2d", seq)
    return m


def _residual_block(c) -> nn.Module:
    m = nn.Module()
    m.add_module("residualblock", _double_conv(c, c))
    return m


def _seq(children: Sequence[Tuple[str, nn.Module]]) -> nn.Module:
    m = nn.Module()
    for n, c in children:
        m.add_module(n, c)
    return m


# ------------------------------------------------------------------------------------------------ storage
class L2Store:
    """Flat fp32 arenas (param, grad) over the network's distinct parameters - the ones the forward uses first, the dead ones behind
    them, so that the optimizer's range [0, live_numel) never touches a parameter torch would leave alone - and the packed copies of
    the 3 x 3 weights the convolution kernels read (forward and flipped / transposed for the data gradient), as engine.ParamStore."""

    def __init__(self, shapes: "OrderedDict[str, Tuple[int, ...]]", live: Sequence[str], convs: Sequence[str], device):
        self.device = torch.device(device)
        self.dtype = self.fwd_dtype = hip.F32
        self.offsets: "OrderedDict[str, Tuple[int, Tuple[int, ...]]]" = OrderedDict()
        off = 0
        live_set = set(live)
        for part in (True, False):
            for k, shp in shapes.items():
                if (k in live_set) == part:
                    self.offsets[k] = (off, tuple(shp))
                    off += rup(max(1, math.prod(shp)), 4)
            if part:
                self.live_numel = off
        self.numel = off
        self.keys = list(shapes)                       # named_parameters() order
        self.live_keys = [k for k in shapes if k in live_set]
        self.data = torch.zeros(off, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=self.device)
        L = hip.lib()
        ck = L.ssr_conv2d_ck(hip.F32, 3)
        self.packed_fwd, self.packed_dgrad, self.pad, self.specs = {}, {}, {}, {}
        items = []
        for name in convs:
            cout, cin, k, _ = shapes[name + ".weight"]
            assert k == 3
            cout_pad, cin_pad = rup(cout, 32), rup(rup(cin, 8), ck)
            cin_pad_o, cout_pad_i = rup(cin, 32), rup(rup(cout, 8), ck)
            pf = torch.zeros(9 * cout_pad * cin_pad, dtype=torch.float32, device=self.device)
            pd = torch.zeros(9 * cin_pad_o * cout_pad_i, dtype=torch.float32, device=self.device)
            self.packed_fwd[name], self.packed_dgrad[name] = pf, pd
            self.pad[name] = (cout_pad, cin_pad, cin_pad_o, cout_pad_i)
            self.specs[name] = ConvSpec(name, cout, cin)
            items.append(PackItem(self.ptr(name + ".weight"), None, pf.data_ptr(), pd.data_ptr(), cout, cin, 3, 3, 1, cout_pad, cin_pad,
                                  cin_pad_o, cout_pad_i, ck, ck, 0))
        self._pack_items = items
        self.pack_table = hip.device_table(items, self.device)

    def tensor(self, key: str, arena: Optional[torch.Tensor] = None) -> torch.Tensor:
        off, shape = self.offsets[key]
        return (self.data if arena is None else arena)[off:off + math.prod(shape)].view(shape)

    def ptr(self, key: str, arena: Optional[torch.Tensor] = None) -> int:
        return (self.data if arena is None else arena).data_ptr() + 4 * self.offsets[key][0]

    def wkey(self, name: str) -> str:
        return name + ".weight"

    def pack(self):
        hip.check(hip.lib().ssr_pack_weights(self.pack_table.data_ptr(), len(self._pack_items), hip.F32, hip.stream_ptr()),
                  "ssr_pack_weights")

    def live_view(self):
        """what optimizers.OptimState sees: the live range of both arenas"""
        return _LiveArena(self)


class _LiveArena:
    def __init__(self, st: L2Store):
        self.device, self.numel = st.device, st.live_numel
        self.data, self.grad = st.data[:st.live_numel], st.grad[:st.live_numel]


# ------------------------------------------------------------------------------------------------ the launch plan
class _Node:
    """an activation: the buffer a PReLU launch wrote (padded or not) and, in the backward, the gradient buffers that flow into it"""

    def __init__(self, buf: torch.Tensor, N: int, C: int, pad: int, group: int = 1, fold: int = 1):
        self.buf, self.N, self.C, self.pad, self.group, self.fold = buf, N, C, pad, group, fold
        self.grads: List[Tuple[torch.Tensor, int]] = []        # (gradient buffer laid out like `buf`, its pad)


class L2Plan:
    """Static launch lists (forward, backward) over preallocated NHWC buffers for one (B, H, W) of SRCNN or HighResNet."""

    def __init__(self, net: "_L2Net", B: int, H: int, W: int, training: bool):
        self.net, self.B, self.H, self.W, self.training = net, B, H, W, training
        st = self.st = net._store
        dev = st.device
        self.keep = []          # descriptors (they hold raw addresses only)
        self._bufs = []         # every device buffer a descriptor points into: the plan owns them for as long as it can be launched
        kw = net.kwargs
        R, h, Cin = kw["revisits"], kw["hidden_channels"], kw["in_channels"]
        z, Co = kw["zoom_factor"], kw["out_channels"]
        self.zoom, self.Co = z, Co
        N0 = B * R
        f32 = dict(dtype=torch.float32, device=dev)
        self.one = torch.ones(1, **f32)
        self.partial = torch.zeros(hip.L2_SLOTS, dtype=torch.float64, device=dev)
        self.fwd, self.bwd = Launcher(), Launcher()
        self._bwd_steps = []                 # closures appended in forward order, replayed in reverse to build the backward
        self.sites: List[Tuple[torch.Tensor, Tuple[int, int, int, int]]] = []    # (packed mask words, NCHW shape) per dropout site
        self.wbatches: List[WgradBatch] = []
        self._wb = None
        self._used_dw = set()

        # input: NCHW -> NHWC (8 channels), then its reflect-padded copy (a PReLU launch with slope 1 is the identity)
        cin8 = rup(Cin, 8)
        self.x_raw = torch.zeros(N0, H, W, cin8, **f32)
        x_pad = _Node(self._zeros(N0, H + 2, W + 2, cin8), N0, cin8, 1)
        self._prelu_fwd(self.x_raw, N0, cin8, self.one.data_ptr(), None, x_pad)

        enc = "encoder.doubleconv2d."
        if net.ARCH == "SRCNN":
            fused = _Node(self._zeros(B, H + 2, W + 2, R * h), N0, h, 1, group=R, fold=1)
            self._double_conv(enc, x_pad, N0, cin8, h, fused, first=True)
            fused_in = _Node(fused.buf, B, R * h, 1)
            fused_in.grads = fused.grads
            nres = kw["residual_layers"]
            y = self._new_node(B, h, pad=1 if nres else 0)
            self._double_conv("doubleconv2d.doubleconv2d.", fused_in, B, R * h, h, y)
            for i in range(nres):
                y2 = self._new_node(B, h, pad=1 if i + 1 < nres else 0)
                self._double_conv(f"residualblocks.{i}.residualblock.doubleconv2d.", y, B, h, h, y2, res=y)
                y = y2
        else:
            levels = net.levels
            Rp = 1 << levels
            if levels == 0:
                y = self._new_node(N0, h, pad=0)
                self._double_conv(enc, x_pad, N0, cin8, h, y, first=True)
            else:
                # level input [B * Rp / 2, 2h]: revisit r of image b -> image b * Rp/2 + r % (Rp/2), channel half r / (Rp/2); the
                # zero revisits appended to a revisit count that is no power of two are the slots no launch ever writes
                half = Rp // 2
                cur = _Node(self._zeros(B * half, H + 2, W + 2, 2 * h), N0, h, 1, group=R, fold=half)
                self._double_conv(enc, x_pad, N0, cin8, h, cur, first=True)
                for lv in range(levels):
                    n_l = B * half
                    p = "fusion.fusion.0.fuse."
                    xin = _Node(cur.buf, n_l, 2 * h, 1)
                    xin.grads = cur.grads
                    yb = self._new_node(n_l, 2 * h, pad=1)
                    self._double_conv(p + "0.residualblock.doubleconv2d.", xin, n_l, 2 * h, 2 * h, yb, res=xin)
                    if lv + 1 < levels:
                        nh = half // 2
                        nxt = _Node(self._zeros(B * nh, H + 2, W + 2, 2 * h), n_l, h, 1, group=half, fold=nh)
                    else:
                        nh, nxt = 0, self._new_node(n_l, h, pad=0)
                    self._conv_prelu(p + "1", p + "3.weight", yb, n_l, 2 * h, h, nxt, drop=False)
                    cur, half = nxt, nh
                y = cur
        # PixelShuffle tail
        self.out = torch.zeros(B, z * H, z * W, 8, **f32)
        self.d_out = torch.zeros(B, z * H, z * W, 8, **f32)
        t = SrTailDesc()
        t.N, t.H, t.W, t.hidden, t.zoom, t.Cout = B, H, W, h, z, Co
        t.x = view(y.buf)
        u = "sr.upsample."
        t.w1, t.b1, t.s1 = st.ptr(u + "1.weight"), st.ptr(u + "1.bias"), st.ptr(u + "3.weight")
        t.w2, t.b2, t.s2 = st.ptr(u + "4.weight"), st.ptr(u + "4.bias"), st.ptr(u + "6.weight")
        t.y = view(self.out)
        self.keep.append(t)
        self.fwd.add(hip.lib().ssr_sr_tail_fwd, C.byref(t), what="sr tail fwd")
        if training:
            g = st.grad
            dy = self._zeros(*y.buf.shape)
            y.grads.append((dy, 0))
            t.gy, t.dx = view(self.d_out), view(dy)
            t.dw1, t.db1, t.ds1 = st.ptr(u + "1.weight", g), st.ptr(u + "1.bias", g), st.ptr(u + "3.weight", g)
            t.dw2, t.db2, t.ds2 = st.ptr(u + "4.weight", g), st.ptr(u + "4.bias", g), st.ptr(u + "6.weight", g)
            nbytes = hip.lib().ssr_sr_tail_scratch_bytes(B, H, W, h, z, Co)
            self.tail_scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=dev)
            t.scratch = self.tail_scratch.data_ptr()
            self.bwd.add(hip.lib().ssr_sr_tail_bwd, C.byref(t), what="sr tail bwd")
            for step in reversed(self._bwd_steps):
                step()
            self._close_wbatch()

    # ---- building blocks ----
    def _zeros(self, *shape, dtype=torch.float32) -> torch.Tensor:
        """a zeroed device buffer that lives as long as the plan: descriptors, the weight-gradient tables and the backward closures
        refer to buffers by address, so a buffer held by a local name alone would be handed out again by the allocator"""
        t = torch.zeros(*shape, dtype=dtype, device=self.st.device)
        self._bufs.append(t)
        return t

    def _new_node(self, N, Cc, pad) -> _Node:
        return _Node(self._zeros(N, self.H + 2 * pad, self.W + 2 * pad, Cc), N, Cc, pad)

    def _prelu_fwd(self, pre: torch.Tensor, N, Cc, slope_ptr, mask: Optional[torch.Tensor], out: _Node, res: Optional[_Node] = None):
        d = PreluReflectDesc()
        d.N, d.H, d.W, d.C = N, self.H, self.W, Cc
        d.pre, d.slope = view(pre), slope_ptr
        d.mask = mask.data_ptr() if mask is not None else None
        d.group, d.fold = out.group, out.fold
        d.out, d.out_pad = view(out.buf), out.pad
        if res is not None:
            d.res, d.res_pad = view(res.buf), res.pad
        self.keep.append(d)
        self.fwd.add(hip.lib().ssr_prelu_reflect_fwd, C.byref(d), what="prelu / reflect fwd")
        return d

    def _conv_prelu(self, conv: str, slope_key: str, x: _Node, N, cin, cout, out: _Node, drop: bool, res: Optional[_Node] = None,
                    first: bool = False):
        """conv 3x3 (reflect) over node x -> pre; PReLU (+ dropout, + residual) -> node `out`; and the same backwards"""
        st, H, W = self.st, self.H, self.W
        pre = self._zeros(N, H, W, cout)
        d = conv_desc(dtype=hip.F32, x=view(x.buf), N=N, Hi=H + 2, Wi=W + 2, Cin=cin, w=st.packed_fwd[conv].data_ptr(),
                      CoutPad=st.pad[conv][0], bias=st.ptr(conv + ".bias"), KH=3, pad_y=0, Gh=H, Gw=W, Cout=cout, y=view(pre))
        self.keep.append(d)
        self.fwd.add(hip.lib().ssr_conv2d, C.byref(d), what=f"conv fwd {conv}")
        mask = None
        if drop and self.training:
            mask = self._zeros(mask_words(N * H * W * cout), dtype=torch.int32)
            self.sites.append((mask, (N, cout, H, W)))
        self._prelu_fwd(pre, N, cout, st.ptr(slope_key), mask, out, res)
        if not self.training:
            return

        def backward():
            dpre = self._zeros(N, H, W, cout)
            b = PreluReflectDesc()
            b.N, b.H, b.W, b.C = N, H, W, cout
            b.pre, b.slope = view(pre), st.ptr(slope_key)
            b.mask = mask.data_ptr() if mask is not None else None
            b.group, b.fold = out.group, out.fold
            assert 1 <= len(out.grads) <= 2, (conv, len(out.grads))
            b.g, b.g_pad = view(out.grads[0][0]), out.grads[0][1]
            if len(out.grads) == 2:
                b.g2, b.g2_pad = view(out.grads[1][0]), out.grads[1][1]
            b.dpre, b.dslope, b.partial = view(dpre), st.ptr(slope_key, st.grad), self.partial.data_ptr()
            if res is not None:
                # x + DoubleConv(x): the total gradient of this output also flows straight into x
                if len(out.grads) == 1:
                    res.grads.append(out.grads[0])
                else:
                    tsum = self._zeros(N, H, W, cout)
                    b.tsum = view(tsum)
                    res.grads.append((tsum, 0))
            self.keep.append(b)
            self.bwd.add(hip.lib().ssr_prelu_reflect_bwd, C.byref(b), what=f"prelu / reflect bwd {conv}")
            # weight and bias gradient: pad-0 wgrad over the padded input
            self._wgrad(conv, view(x.buf), view(dpre), N, cin)
            if first:
                return
            # data gradient: the full correlation with flipped weights (pad 2) onto the padded grid of x
            gx = self._zeros(*x.buf.shape)
            e = conv_desc(dtype=hip.F32, x=view(dpre), N=N, Hi=H, Wi=W, Cin=rup(cout, 8), w=st.packed_dgrad[conv].data_ptr(),
                          CoutPad=st.pad[conv][2], KH=3, pad_y=2, Gh=H + 2, Gw=W + 2, Cout=st.specs[conv].cin, y=view(gx))
            self.keep.append(e)
            self.bwd.add(hip.lib().ssr_conv2d, C.byref(e), what=f"conv dgrad {conv}")
            x.grads.insert(0, (gx, 1))
        self._bwd_steps.append(backward)

    def _double_conv(self, p: str, x: _Node, N, cin, cout, out: _Node, res: Optional[_Node] = None, first: bool = False):
        mid = self._new_node(N, cout, pad=1)
        self._conv_prelu(p + "0", p + "2.weight", x, N, cin, cout, mid, drop=True, first=first)
        self._conv_prelu(p + "4", p + "6.weight", mid, N, cout, cout, out, drop=True, res=res)

    def _wgrad(self, conv, x: View, dy: View, N, cin):
        """deterministic batches (per-split partials, fixed-order sums); a layer applied more than once - HighResNet's shared fusion
        block - goes into a later batch each time, so that one launch never has two writers of one gradient"""
        st = self.st
        if self._wb is None or conv in self._used_dw:
            self._close_wbatch()
            self._wb = WgradBatch(hip.F32, 3, 1, det=True, device=st.device)
            self._used_dw = set()
        self._used_dw.add(conv)
        self._wb.add(x, dy, N, self.H + 2, self.W + 2, 1, gh=self.H, gw=self.W, alpha=1.0, pad=0, **wgrad_args(st, conv, cin))

    def _close_wbatch(self):
        if self._wb is not None and self._wb.layers:
            self._wb.finalize()
            self._wb.launch(self.bwd)
            self.wbatches.append(self._wb)
        self._wb = None

    # ---- boundary ----
    def load_input(self, x: torch.Tensor, scale: float = 1.0):
        B, R, Cc, H, W = x.shape
        hip.check(hip.lib().ssr_nchw_to_nhwc(x.data_ptr(), B * R, Cc, H, W, view(self.x_raw), hip.F32, 1, 1, scale, hip.stream_ptr()),
                  "ssr_nchw_to_nhwc")

    def read_output(self) -> torch.Tensor:
        z = self.zoom
        y = torch.empty(self.B, self.Co, z * self.H, z * self.W, dtype=torch.float32, device=self.st.device)
        hip.check(hip.lib().ssr_nhwc_to_nchw(view(self.out), hip.F32, y.data_ptr(), self.B, self.Co, z * self.H, z * self.W,
                                             hip.stream_ptr()), "ssr_nhwc_to_nchw")
        return y

    def load_output_grad(self, g: torch.Tensor):
        z = self.zoom
        hip.check(hip.lib().ssr_nchw_to_nhwc(g.data_ptr(), self.B, self.Co, z * self.H, z * self.W, view(self.d_out), hip.F32, 1, 1, 1.0,
                                             hip.stream_ptr()), "ssr_nchw_to_nhwc")

    def set_masks(self, masks: Optional[Sequence[torch.Tensor]]):
        """the keep bits of this forward: the test hook's masks, or the device generator's next draw"""
        if not self.sites:
            return
        if masks is not None:
            assert len(masks) == len(self.sites), f"{len(masks)} dropout masks for {len(self.sites)} sites"
            for (buf, shape), m in zip(self.sites, masks):
                assert tuple(m.shape) == shape, f"dropout mask {tuple(m.shape)} for a site of {shape}"
                buf.copy_(torch.from_numpy(pack_mask_nhwc(m).view("int32")))
            return
        net, L, st = self.net, hip.lib(), hip.stream_ptr()
        for i, (buf, _) in enumerate(self.sites):
            hip.check(L.ssr_dropout_mask(buf.data_ptr(), buf.numel(), net.seed & 0xFFFFFFFFFFFFFFFF, net.drop_step.data_ptr(), i,
                                         1 if i + 1 == len(self.sites) else 0, st), "ssr_dropout_mask")


# ------------------------------------------------------------------------------------------------ the modules
class _L2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, plan, x, masks, *params):
        y = net._run(plan, x, masks)
        ctx.net, ctx.plan, ctx.gen = net, plan, plan.generation
        return y

    @staticmethod
    def backward(ctx, gy):
        net, plan = ctx.net, ctx.plan
        if plan.generation != ctx.gen:
            raise RuntimeError(f"{net.ARCH}: activations of this forward were overwritten by a later forward of the same shape")
        st = net._store
        plan.load_output_grad(gy.reshape(plan.B, plan.Co, gy.shape[-2], gy.shape[-1]).contiguous().float())
        st.grad.zero_()
        plan.bwd.run()
        live = set(st.live_keys)
        return (None, None, None, None, *[st.tensor(k, st.grad).clone() if (need and k in live) else None
                                          for k, need in zip(st.keys, ctx.needs_input_grad[4:])])


class _L2Net(nn.Module):
    ARCH = ""

    def _init_common(self, kw: Dict, compute_dtype):
        check_compute_dtype(compute_dtype)
        check_arch_options(kw)
        self.kwargs = dict(kw)
        self.compute_dtype = compute_dtype
        self.output_size = kw["output_size"]
        self.seed = 0
        self._store: Optional[L2Store] = None
        self._plans: Dict[Tuple, L2Plan] = {}
        self.drop_step = None
        h, R, z = kw["hidden_channels"], kw["revisits"], kw["zoom_factor"]
        cm = h // (z * z)
        self.encoder = _double_conv(kw["in_channels"], h)
        self.mask_encoder = _seq([("1", _double_conv(0, 1))])
        self.doubleconv2d = _double_conv(h * R, h)
        self.residualblocks = _seq([(str(i), _residual_block(h)) for i in range(kw["residual_layers"])])
        self.fusion = _seq([("0", self.doubleconv2d), ("1", self.residualblocks)])
        self.sr = _seq([("upsample", _seq([("1", _conv(cm, cm, 1)), ("3", _Slope()), ("4", _conv(kw["out_channels"], cm, 1)),
                                            ("6", _Slope())]))])

    def manual_seed(self, seed: int):
        """seed of the dropout generator (L2Model passes the option file's manual_seed); the step counter restarts"""
        self.seed = int(seed)
        if self.drop_step is not None:
            self.drop_step.zero_()
        return self

    def live_keys(self) -> List[str]:
        dead = self.DEAD
        return [k for k, _ in self.named_parameters() if not k.startswith(dead)]

    def store(self) -> L2Store:
        p0 = next(self.parameters())
        if not p0.is_cuda:
            raise hip.HipLibraryError(f"{self.ARCH} runs only on the GPU through libssr_hip.so (no CPU path; the CPU statement is "
                                      "l2_reference.py): move it with .to('cuda') / .cuda()")
        st = self._store
        names = [k for k, _ in self.named_parameters()]
        if st is not None and st.device == p0.device and p0.data_ptr() == st.ptr(names[0]):
            return st
        hip.lib()
        shapes = OrderedDict((k, tuple(p.shape)) for k, p in self.named_parameters())
        live = self.live_keys()
        convs = [k[:-len(".weight")] for k in live if k.endswith(".weight") and len(shapes[k]) == 4 and shapes[k][-1] == 3]
        st = L2Store(shapes, live, convs, p0.device)
        with torch.no_grad():
            for key, p in self.named_parameters():
                if p.numel():
                    st.tensor(key).copy_(p.data)
                    p.data = st.tensor(key)
        self._store = st
        self._plans.clear()
        if self.drop_step is None or self.drop_step.device != p0.device:
            self.drop_step = torch.zeros(1, dtype=torch.int32, device=p0.device)
        return st

    def plan(self, B, H, W, training) -> L2Plan:
        key = (B, H, W, bool(training))
        if key not in self._plans:
            self._plans[key] = L2Plan(self, B, H, W, bool(training))
        return self._plans[key]

    def _run(self, plan: L2Plan, x, masks):
        self._store.pack()
        plan.load_input(x.detach().contiguous().float())
        plan.set_masks(masks)
        plan.fwd.run()
        plan.generation = getattr(plan, "generation", 0) + 1
        return plan.read_output()[:, None]

    def check_input(self, x, mask=None):
        if mask is not None:
            raise NotImplementedError("mask: the mask encoder (mask_channels > 0) is outside this path")
        if x.dim() != 5 or x.shape[1] != self.kwargs["revisits"] or x.shape[2] != self.kwargs["in_channels"]:
            raise ValueError(f"{self.ARCH}: input {tuple(x.shape)}, expected [B, {self.kwargs['revisits']}, {self.kwargs['in_channels']}, H, W]")
        H, W = x.shape[-2:]
        if H < 2 or W < 2:
            raise ValueError(f"{self.ARCH}: reflect padding needs H, W >= 2")
        if self.RESIZES:
            check_output_size(self.output_size, self.kwargs["zoom_factor"], H, W)
        self.store()
        if not x.is_cuda:
            raise hip.HipLibraryError(f"{self.ARCH} runs only on the GPU through libssr_hip.so (no CPU path)")

    def forward(self, x, y=None, mask=None, dropout_masks=None):
        self.check_input(x, mask)
        B, _, _, H, W = x.shape
        train = self.training
        if dropout_masks is not None and not train:
            raise ValueError("dropout_masks: eval() makes Dropout the identity")
        params = list(self.parameters())
        need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if not need and not train:
            return self._run(self.plan(B, H, W, False), x, None)
        if need and not train:
            raise NotImplementedError(f"{self.ARCH}: gradients through eval() (Dropout off): call .train(), or wrap the forward in "
                                      "torch.no_grad()")
        plan = self.plan(B, H, W, True)      # training-mode forwards keep what the backward reads (pre-activations, masks)
        if not need:
            return self._run(plan, x, dropout_masks)
        return _L2Fn.apply(self, plan, x, dropout_masks, *params)


@ARCH_REGISTRY.register()
class SRCNN(_L2Net):
    ARCH, DEAD, RESIZES = "SRCNN", ("mask_encoder.",), True

    def __init__(self, in_channels, mask_channels, revisits, hidden_channels, out_channels, kernel_size, residual_layers, output_size,
                 zoom_factor, sr_kernel_size, use_reference_frame=False, compute_dtype="fp32", **kws):
        super().__init__()
        self._init_common(dict(in_channels=in_channels, mask_channels=mask_channels, revisits=revisits, hidden_channels=hidden_channels,
                               out_channels=out_channels, kernel_size=kernel_size, residual_layers=residual_layers,
                               output_size=output_size, zoom_factor=zoom_factor, sr_kernel_size=sr_kernel_size,
                               use_reference_frame=use_reference_frame), compute_dtype)


@ARCH_REGISTRY.register()
class HighResNet(_L2Net):
    ARCH, DEAD, RESIZES = "HighResNet", ("mask_encoder.", "doubleconv2d.", "residualblocks."), False

    def __init__(self, skip_paddings=True, compute_dtype="fp32", **kws):
        super().__init__()
        kws.setdefault("use_reference_frame", False)
        need = ("in_channels", "mask_channels", "revisits", "hidden_channels", "out_channels", "kernel_size", "residual_layers",
                "output_size", "zoom_factor", "sr_kernel_size")
        for k in need:
            if k not in kws:
                raise TypeError(f"HighResNet: missing constructor argument {k!r}")
        self._init_common({k: kws[k] for k in need + ("use_reference_frame",)}, compute_dtype)
        self.skip_paddings = skip_paddings
        h, R = self.kwargs["hidden_channels"], self.kwargs["revisits"]
        self.levels = max(0, (R - 1).bit_length())
        block = _seq([("fuse", _seq([("0", _residual_block(2 * h)), ("1", _conv(h, 2 * h)), ("3", _Slope())]))])
        self.fusion = _seq([("fusion", _seq([(str(i), block) for i in range(self.levels)]))])
