"""The LPIPS validation metric of the shipped option files (`lpips: {type: calculate_lpips, lpips_model: vgg}`,
esrgan_s2naip_urban.yml:154-186; /root/reference/ssr/metrics/lpips.py:7-21) on the device.

The reference is 21 lines around the third-party `lpips` package, which is not a dependency of this package.  What is built here is
that package's documented network (version 0.1, net 'vgg', eval mode), written from its definition and NOT executed against the
package itself: every statement below that rests on the package or on BasicSR is marked [recalled] ("LPIPS metric").

    d(x0, x1) = sum_k mean_{h,w} sum_c w_k[c] * (n(F_k(x0)) - n(F_k(x1)))^2,     n(F) = F / (sqrt(sum_c F^2) + 1e-10) per pixel

    scaling layer   x_c = (in_c - shift_c) / scale_c, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)          [recalled]
    F_k             the post-ReLU outputs of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 of torchvision's VGG16 `features` [recalled]
    w_k             the bias-free 1x1 convolution `lin{k}.model.1.weight` [1, C_k, 1, 1] (dropout in front: inactive)      [recalled]

Two quirks of the reference are the defaults here, because users compare against numbers produced that way:
  * it is called with what `tensor2img` returns, which is BGR [recalled], so the network's channel 0 sees blue (`rgb: true` undoes it);
  * it scales by /255 only and calls LPIPS with its default normalize=False, so the network sees [0, 1], not the [-1, 1] it was
    trained on (`normalize: true` maps to [-1, 1]).

The VGG16 forward runs on the conv kernels in exact fp32 whatever the model's compute_dtype (a reported number, and validation is
not the hot loop); the scaling layer and the per-tap arithmetic are csrc/lpips.hip.

The second backbone of the reference's function, `lpips_model: alexnet` (net 'alex' of the package, its default), shares the scaling
layer, the `lin{k}` layers and the formula; only F_k differs:

    F_k             the post-ReLU outputs of the five convolutions of torchvision's AlexNet `features` (indices 0, 3, 6, 8, 10):
                    3->64 11x11 s4 p2 | maxpool 3x3 s2 | 64->192 5x5 p2 | maxpool 3x3 s2 | 192->384, 384->256, 256->256 3x3 p1      [recalled]
                    (the package's slices features[0:2], [2:5], [5:8], [8:10], [10:12])                                          [recalled]

Its first two convolutions and its pooling are csrc/conv_direct.hip (ssr_conv_direct, ssr_maxpool3s2_fwd); the three 3x3 layers run
through ssr_conv2d in exact fp32 like VGG's.  Every function below takes the backbone as `net` ('vgg' by default, 'alex').

The two backbones themselves - layer records, geometry, specs, random weights, the forward's launches - are cnn_backbone.py, shared
with the perceptual loss's VGG19.

    vgg16_layers / vgg16_specs     the layer table (cnn_backbone's records as plain tuples)
    alexnet_layers / alexnet_specs / alexnet_tap_sizes      the second backbone's
    load_lpips_state               torchvision + lpips files, one lpips state_dict, or the flat layout -> flat layout
    lpips_random_state             random weights of the same architecture (tests, throughput runs)
    lpips_reference                the definition in torch on the CPU
    LPIPSPlan / LPIPSModel         the static launch list for one (N, H, W) / the weights on the device and their plans
    lpips_distance                 uint8 NHWC device images -> float64 [N] on the host
    calculate_lpips                the entry of metrics.METRICS
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import cnn_backbone as CB, engine, hip
from .cnn_backbone import ALEXNET_LAYERS, VGG16_BLOCKS          # the backbones are written there
from .hip import view

LPIPS_PRETRAIN_PATH = "experiments/pretrained_models/lpips_vgg.pth"
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
LPIPS_EPS = 1e-10
LPIPS_TAPS = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
LPIPS_ALEX_PRETRAIN_PATH = "experiments/pretrained_models/lpips_alex.pth"
LPIPS_ALEX_TAPS = tuple(l.name for l in ALEXNET_LAYERS)          # every layer is a tap       [recalled]
ALEXNET_MIN_SIDE = 31              # the smallest side that leaves a pixel behind both poolings: taps of 7, 3, 1, 1, 1
# keys of a `calculate_lpips` metric entry: the reference's **kwargs swallows the first four
_IGNORED_KEYS = ("crop_border", "test_y_channel", "input_order", "better", "type")
_OUR_KEYS = ("lpips_model", "lpips_weights", "vgg16_path", "alexnet_path", "lin_path", "rgb", "normalize")
_NETS = {"vgg": "vgg", "vgg16": "vgg", "alex": "alex", "alexnet": "alex"}


def _net(net: str) -> str:
    """'vgg' | 'alex' from an option value (`lpips_model: vgg | alexnet`) or the package's name (net='vgg' | 'alex')"""
    if net not in _NETS:
        raise NotImplementedError(f"metric type 'calculate_lpips': lpips_model={net!r}: the reference offers 'alexnet' and 'vgg'")
    return _NETS[net]


def vgg16_layers():
    """[(name 'convB_J', torchvision features index, cin, cout, pooled_before)]"""
    return [(l.name, l.idx, l.cin, l.cout, bool(l.pool)) for l in CB.vgg_layers(VGG16_BLOCKS)]


def vgg16_specs():
    # no backward here: the transposed packing of the weights is left out
    return CB.conv_specs(CB.vgg_layers(VGG16_BLOCKS), dgrad_packed=False)


def alexnet_layers():
    """[(name 'convJ', torchvision features index, cin, cout, kernel, stride, pad, pooled_before)]"""
    return [tuple(l[:7]) + (bool(l.pool),) for l in ALEXNET_LAYERS]


def alexnet_specs():
    """the 3x3 layers, which ssr_conv2d runs (conv1 and conv2 go through ssr_conv_direct and are not in a ParamStore)"""
    return CB.conv_specs(ALEXNET_LAYERS, dgrad_packed=False)


def alexnet_tap_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """(h, w) of the five taps of an H x W image; ValueError below 31 (no divisibility is needed above it)"""
    if H < ALEXNET_MIN_SIDE or W < ALEXNET_MIN_SIDE:
        raise ValueError(f"LPIPS (AlexNet: 11x11 stride-4 convolution, two 3x3 stride-2 poolings) needs H and W >= {ALEXNET_MIN_SIDE}, "
                         f"got {H} x {W}")
    return CB.tap_sizes(ALEXNET_LAYERS, H, W)


def _layers(net: str = "vgg") -> List[CB.Layer]:
    return list(ALEXNET_LAYERS) if _net(net) == "alex" else CB.vgg_layers(VGG16_BLOCKS)


def _tap_names(net: str = "vgg") -> Tuple[str, ...]:
    return LPIPS_ALEX_TAPS if _net(net) == "alex" else LPIPS_TAPS


def _tap_widths(net: str = "vgg") -> List[int]:
    return [l.cout for l in _layers(net) if l.name in _tap_names(net)]


def lpips_random_state(seed: int = 0, net: str = "vgg") -> Dict[str, torch.Tensor]:
    """Flat layout.  VGG: convolutions as torchvision's VGG._initialize_weights (kaiming_normal_(fan_out, relu), zero bias).
    AlexNet: torchvision's AlexNet keeps nn.Conv2d's default, weights and biases from U(-b, b), b = 1 / sqrt(fan_in) [recalled], so
    its biases are not zero.  `lin` weights from U[0, 1) (the package's are non-negative: the metric is a weighted sum of squares)."""
    g = torch.Generator().manual_seed(seed)
    sd = CB.random_conv_state(CB.conv_shapes(_layers(net)), g, kaiming=_net(net) != "alex")
    for k, c in enumerate(_tap_widths(net)):
        sd[f"lin{k}"] = torch.rand(c, generator=g)
    return sd


def load_lpips_state(backbone_path: str, lin_path: Optional[str] = None, net: str = "vgg") -> Dict[str, torch.Tensor]:
    """-> {features.{idx}.weight / .bias (13 convolutions), lin{k} [C_k] (5 taps)}, float32, from any of   [recalled]
      * torchvision's vgg16-397923af.pth (`features.{idx}.*`) + the lpips package's weights/v0.1/vgg.pth (`lin{k}.model.1.weight`);
      * one file saved from lpips.LPIPS(net='vgg').state_dict(): `net.slice{s}.{idx}.*` with the same torchvision indices and
        `lin{k}.model.1.weight` (the duplicate `lins.{k}.*` and the `scaling_layer.*` keys are ignored);
      * the flat layout itself.
    net='alex': the same three with torchvision's alexnet-owt-7be5be79.pth (`features.{0,3,6,8,10}.*`, 5 convolutions), the package's
    weights/v0.1/alex.pth and lpips.LPIPS(net='alex').state_dict() (`net.slice{1..5}.{0,3,6,8,10}.*`).                     [recalled]
    KeyError / ValueError name the key that is missing / mis-shaped; the other backbone's file fails so on its first key."""
    sd = dict(CB.load_features_state(backbone_path))
    lin_sd = CB.load_features_state(lin_path) if lin_path else {}
    out = {}
    for conv, wshape in CB.conv_shapes(_layers(net)):
        idx = conv[len("features."):]
        for leaf, shape in (("weight", wshape), ("bias", wshape[:1])):
            key = f"{conv}.{leaf}"
            cands = [key] + [f"net.slice{s}.{idx}.{leaf}" for s in range(1, 6)]
            src = next((c for c in cands if c in sd), None)
            if src is None:
                raise KeyError(f"{key} (or net.slice{{s}}.{idx}.{leaf}) not in {backbone_path}")
            t = sd[src]
            if tuple(t.shape) != shape:
                raise ValueError(f"{src}: shape {tuple(t.shape)}, expected {shape}")
            out[key] = t.detach().to(torch.float32).clone()
    for k, c in enumerate(_tap_widths(net)):
        key = f"lin{k}"
        cands = [(lin_sd, f"lin{k}.model.1.weight"), (lin_sd, key), (sd, key), (sd, f"lin{k}.model.1.weight")]
        hit = next(((d, n) for d, n in cands if n in d), None)
        if hit is None:
            raise KeyError(f"{key} (or lin{k}.model.1.weight) not in {lin_path or backbone_path}")
        t = hit[0][hit[1]]
        if tuple(t.shape) not in ((c,), (1, c, 1, 1)):
            raise ValueError(f"{hit[1]}: shape {tuple(t.shape)}, expected (1, {c}, 1, 1)")
        out[key] = t.detach().to(torch.float32).reshape(c).clone()
    return out


# ---------------------------------------------------------------- the definition, on the CPU
def lpips_scaled_input(img_u8: torch.Tensor, bgr: bool = True, normalize: bool = False, dtype=torch.float64) -> torch.Tensor:
    """uint8 [N, H, W, 3] RGB -> the scaling layer's output, NCHW.  In float32 this is the operation order of ssr_lpips_input."""
    x = torch.as_tensor(img_u8)
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3, "uint8 [N, H, W, 3]"
    x = x.cpu().to(dtype) / 255
    if bgr:
        x = x.flip(-1)
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(LPIPS_SHIFT, dtype=torch.float32).to(dtype)       # the package keeps both as float32 buffers [recalled]
    scale = torch.tensor(LPIPS_SCALE, dtype=torch.float32).to(dtype)
    return ((x - shift) / scale).permute(0, 3, 1, 2).contiguous()


def tap_features(x: torch.Tensor, state: Dict[str, torch.Tensor], net: str = "vgg") -> Dict[str, torch.Tensor]:
    """the five post-ReLU taps of an NCHW input"""
    feats = {}
    for l in _layers(net):
        if l.pool:
            x = F.max_pool2d(x, l.pool, 2)
        x = F.relu(F.conv2d(x, state[f"features.{l.idx}.weight"].to(x.dtype), state[f"features.{l.idx}.bias"].to(x.dtype), stride=l.stride,
                            padding=l.pad))
        if l.name in _tap_names(net):
            feats[l.name] = x
    return feats


def lpips_from_features(feats0: Dict[str, torch.Tensor], feats1: Dict[str, torch.Tensor], lins: Dict[str, torch.Tensor]) -> torch.Tensor:
    """step 3 and 4 of the definition for any set of taps: feats*[name] is [N, C, H, W] (post-ReLU), lins[name] is [C] -> [N]"""
    total = None
    for name, f0 in feats0.items():
        f1, w = feats1[name], lins[name].to(f0.dtype).reshape(1, -1, 1, 1)
        n0 = f0 / (f0.pow(2).sum(dim=1, keepdim=True).sqrt() + LPIPS_EPS)
        n1 = f1 / (f1.pow(2).sum(dim=1, keepdim=True).sqrt() + LPIPS_EPS)
        d = (w * (n0 - n1) ** 2).sum(dim=1).mean(dim=(1, 2))
        total = d if total is None else total + d
    return total


def lpips_reference(a_u8, b_u8, state: Dict[str, torch.Tensor], bgr: bool = True, normalize: bool = False,
                    dtype=torch.float64, net: str = "vgg") -> torch.Tensor:
    """LPIPS(net='vgg' | 'alex', version='0.1') of uint8 [N, H, W, 3] RGB image pairs as the reference feeds it (module docstring) -> [N]"""
    with torch.no_grad():
        f0 = tap_features(lpips_scaled_input(a_u8, bgr, normalize, dtype), state, net)
        f1 = tap_features(lpips_scaled_input(b_u8, bgr, normalize, dtype), state, net)
        return lpips_from_features(f0, f1, {t: state[f"lin{k}"] for k, t in enumerate(_tap_names(net))})


# ---------------------------------------------------------------- the device path
class LPIPSPlan:
    """One static launch list for N image pairs of H x W: ssr_lpips_input for both images (one batch of 2N), the 13 convolutions
    with the ReLU epilogue (the tapped ones stored before their ReLU), ssr_relu_maxpool2_fwd behind taps 1-4, five ssr_lpips_layer.
    The ParamStore is the exact fp32 mode's; `store` shares one (already loaded and packed) between the plans of a LPIPSModel.
    net='alex', any H, W >= 31: conv1 and conv2 through ssr_conv_direct, ssr_maxpool3s2_fwd in front of conv2 and conv3, conv3..5
    through ssr_conv2d, every tap stored AFTER its ReLU, five ssr_lpips_layer with relu = 0.  `direct`: {layer name: (weights
    [K*K][Cin][Cout], bias)} on the device (cnn_backbone.append_forward), empty for VGG."""

    def __init__(self, N: int, H: int, W: int, state: Optional[Dict[str, torch.Tensor]], device="cuda", bgr: bool = True,
                 normalize: bool = False, store=None, lins: Optional[torch.Tensor] = None, net: str = "vgg", direct=None):
        self.net = _net(net)
        alex = self.net == "alex"
        if alex and N <= 0:
            raise ValueError(f"LPIPS needs at least one image pair, got N = {N}")
        if alex:
            alexnet_tap_sizes(H, W)                      # ValueError below 31
        elif N <= 0 or H <= 0 or W <= 0 or H % 16 or W % 16:
            raise ValueError(f"LPIPS (VGG16, four poolings) needs H and W divisible by 16, got {N} x {H} x {W}")
        dev = torch.device(device)
        self.N, self.H, self.W = N, H, W
        if store is None:
            store, lins, direct = _device_weights(state, dev, self.net)
        self.store, self.lins, self.direct = store, lins, direct or {}
        lib = hip.lib()
        B = 2 * N
        z = lambda *s: torch.zeros(B, *s, dtype=torch.float32, device=dev)      # noqa: E731
        self.a_u8 = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
        self.b_u8 = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
        self.xn = z(H, W, 8)
        self._shift = (C.c_float * 3)(*LPIPS_SHIFT)
        self._scale = (C.c_float * 3)(*LPIPS_SCALE)
        self._perm = (C.c_int32 * 3)(*((2, 1, 0) if bgr else (0, 1, 2)))
        cb = engine._ConvBuilder(store, B)
        self._cb = cb
        L = engine.Launcher()
        npix = N * H * W
        L.add(lib.ssr_lpips_input, self.a_u8.data_ptr(), view(self.xn[:N]), hip.F32, npix, self._shift, self._scale, self._perm,
              1 if normalize else 0, what="lpips input (image 1)")
        L.add(lib.ssr_lpips_input, self.b_u8.data_ptr(), view(self.xn[N:]), hip.F32, npix, self._shift, self._scale, self._perm,
              1 if normalize else 0, what="lpips input (image 2)")
        layers, tapped = _layers(self.net), _tap_names(self.net)
        self.acts, self.pooled = CB.forward_buffers(layers, H, W, z, tapped, not alex)
        _, taps = CB.append_forward(L, cb, lib, layers, self.xn, H, W, B, hip.F32, tapped, self.acts.__getitem__, self.pooled, not alex,
                                    self.direct)
        self._add_taps(L, taps, relu=0 if alex else 1)
        self.launcher = L

    def _add_taps(self, L, taps, relu: int):
        """the five ssr_lpips_layer launches over self.acts; partials: per tap [N][nblk] doubles, one buffer, one download"""
        lib, N = hip.lib(), self.N
        self.slices, off, woff = [], 0, 0
        for name, hw, c in taps:
            nblk = lib.ssr_lpips_layer_blocks(N, hw, c)
            hip.check(min(nblk, 0), f"ssr_lpips_layer_blocks {name}")
            self.slices.append((off, nblk))
            off += N * nblk
        self.partial = torch.zeros(off, dtype=torch.float64, device=self.lins.device)
        for (name, hw, c), (poff, nblk) in zip(taps, self.slices):
            f = self.acts[name]
            L.add(lib.ssr_lpips_layer, view(f[:N]), view(f[N:]), self.lins.data_ptr() + 4 * woff, hip.F32, N, hw, c, relu,
                  self.partial.data_ptr() + 8 * poff, what=f"lpips layer {name}")
            woff += c

    def run(self, a_u8: torch.Tensor, b_u8: torch.Tensor) -> torch.Tensor:
        """-> float64 [N] on the host (one download: the partials, added in index order per tap, taps in order)"""
        self.a_u8.copy_(a_u8)
        self.b_u8.copy_(b_u8)
        self.launcher.run()
        p = self.partial.cpu().numpy()
        total = 0.0
        for off, nblk in self.slices:
            total = total + p[off:off + self.N * nblk].reshape(self.N, nblk).cumsum(axis=1)[:, -1]
        return torch.from_numpy(total.copy())


def _device_weights(state: Dict[str, torch.Tensor], dev, net: str = "vgg"):
    """-> (ParamStore of the backbone's 3x3 convolutions in the exact fp32 mode, loaded and packed; the five lin vectors as one fp32
    tensor; `direct`).  `direct` is empty for VGG; AlexNet: {layer: (weights [K*K][CinPad][Cout], bias)} in ssr_conv_direct's layout
    for all five layers, permuted here in torch: conv1's 3 input channels padded with zero weights to the 8 channels ssr_lpips_input
    writes."""
    net = _net(net)
    widths = _tap_widths(net)
    for k, c in enumerate(widths):
        if f"lin{k}" not in state:
            raise KeyError(f"lin{k}")
        if tuple(state[f"lin{k}"].shape) != (c,):
            raise ValueError(f"lin{k}: shape {tuple(state[f'lin{k}'].shape)}, expected ({c},)")
    direct = {}
    for l in ALEXNET_LAYERS if net == "alex" else ():
        cout, cin, k, conv = l.cout, l.cin, l.k, f"features.{l.idx}"
        for key, shape in ((conv + ".weight", (cout, cin, k, k)), (conv + ".bias", (cout,))):
            if key not in state:
                raise KeyError(key)
            if tuple(state[key].shape) != shape:
                raise ValueError(f"{key}: shape {tuple(state[key].shape)}, expected {shape}")
        wd = torch.zeros(k * k, -(-cin // 8) * 8, cout, dtype=torch.float32)
        wd[:, :cin] = state[conv + ".weight"].detach().to(torch.float32).permute(2, 3, 1, 0).reshape(k * k, cin, cout)
        direct[l.name] = (wd.to(dev), state[conv + ".bias"].detach().to(torch.float32).contiguous().to(dev))
    store = engine.ParamStore(CB.conv_specs(_layers(net), dgrad_packed=False), hip.F32, device=dev)
    store.load_state_dict(state)
    store.pack()
    lins = torch.cat([state[f"lin{k}"].to(torch.float32) for k in range(len(widths))]).to(dev)
    return store, lins, direct


class LPIPSModel:
    """The weights of one backbone on the device and the plans that use them, cached per (N, H, W, bgr, normalize)."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda", net: str = "vgg"):
        self.device = torch.device(device)
        self.net = _net(net)
        self.store, self.lins, self.direct = _device_weights(state, self.device, self.net)
        self.plans: Dict[Tuple, LPIPSPlan] = {}

    def plan(self, N: int, H: int, W: int, bgr: bool = True, normalize: bool = False) -> LPIPSPlan:
        key = (N, H, W, bool(bgr), bool(normalize))
        if key not in self.plans:
            self.plans[key] = LPIPSPlan(N, H, W, None, self.device, bgr=bgr, normalize=normalize, store=self.store, lins=self.lins,
                                        net=self.net, direct=self.direct)
        return self.plans[key]


def lpips_distance(a_u8: torch.Tensor, b_u8: torch.Tensor, model: LPIPSModel, bgr: bool = True, normalize: bool = False) -> torch.Tensor:
    """a_u8, b_u8: uint8 [N, H, W, 3] RGB device tensors as `tensor2img_u8` gives them -> float64 [N] on the host.  The backbone is
    the model's."""
    if not (a_u8.shape == b_u8.shape and a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.is_cuda and b_u8.is_cuda):
        raise ValueError(f"Image shapes are different: {tuple(a_u8.shape)}, {tuple(b_u8.shape)} (uint8 device tensors)")
    if a_u8.dim() != 4 or a_u8.shape[-1] != 3:
        raise ValueError(f"LPIPS needs uint8 [N, H, W, 3] images, got {tuple(a_u8.shape)}")
    n, h, w, _ = a_u8.shape
    return model.plan(n, h, w, bgr, normalize).run(a_u8, b_u8)


# ---------------------------------------------------------------- the metric entry
_MODELS: Dict[Tuple, LPIPSModel] = {}
# per backbone: (option value, the backbone key, the other backbone's key, environment variable, default file, the package's net name,
#                torchvision's file, the package's lin file)
_BACKBONES = {
    "vgg": ("vgg", "vgg16_path", "alexnet_path", "SSR_LPIPS_WEIGHTS", LPIPS_PRETRAIN_PATH, "vgg", "vgg16-397923af.pth", "vgg.pth"),
    "alex": ("alexnet", "alexnet_path", "vgg16_path", "SSR_LPIPS_ALEX_WEIGHTS", LPIPS_ALEX_PRETRAIN_PATH, "alex", "alexnet-owt-7be5be79.pth",
             "alex.pth"),
}


def check_lpips_opt(lpips_model="vgg", **kw) -> Tuple[str, Optional[str]]:
    """Validates the keys of a `calculate_lpips` entry and finds the weights -> (backbone or combined file, lin file or None).
    Touches no device: the model plugin calls it before the first validation image is processed."""
    if lpips_model not in ("vgg", "alexnet"):             # the reference's two branches, by their names there
        raise NotImplementedError(f"metric type 'calculate_lpips': lpips_model={lpips_model!r}: the reference offers 'alexnet' and 'vgg'")
    net = _net(lpips_model)
    model, bkey, other, env, default, pkg, tv_file, lin_file = _BACKBONES[net]
    for k in kw:
        if k not in _IGNORED_KEYS and k not in _OUR_KEYS:
            raise NotImplementedError(f"metric type 'calculate_lpips': option {k!r} (have {sorted(_OUR_KEYS)})")
    if kw.get(other):
        raise ValueError(f"metric type 'calculate_lpips': {other} belongs to the other backbone: lpips_model={model!r} takes {bkey} + lin_path")
    combined, backbone, lin = kw.get("lpips_weights"), kw.get(bkey), kw.get("lin_path")
    if combined and (backbone or lin):
        raise ValueError(f"metric type 'calculate_lpips': give lpips_weights (one combined file) or {bkey} + lin_path, not both")
    if bool(backbone) != bool(lin):
        raise ValueError(f"metric type 'calculate_lpips': {bkey} and lin_path go together (the backbone and the lpips package's linear layers)")
    for key, path in (("lpips_weights", combined), (bkey, backbone), ("lin_path", lin)):
        if path and not os.path.exists(path):
            raise FileNotFoundError(f"metric type 'calculate_lpips': {key}={path!r} does not exist")
    if combined:
        return os.path.abspath(combined), None
    if backbone:
        return os.path.abspath(backbone), os.path.abspath(lin)
    for cand in (os.environ.get(env), default):
        if cand and os.path.exists(cand):
            return os.path.abspath(cand), None
    raise NotImplementedError(
        "metric type 'calculate_lpips': no LPIPS weights found" + ("" if net == "vgg" else f" for lpips_model={model!r}") +
        ".  Put them in one of three places: the metric's options (`lpips_weights: "
        f"<file saved from lpips.LPIPS(net='{pkg}').state_dict()>`, or `{bkey}: <torchvision {tv_file}>` + `lin_path: <lpips "
        f"weights/v0.1/{lin_file}>`), the environment variable {env}=<combined file>, or {default}.  "
        "There is no silent random network: a metric from random weights is not LPIPS")


def calculate_lpips(img, img2, lpips_model="vgg", **kw) -> float:
    """One image pair per call (uint8 [1, H, W, 3] or [H, W, 3] RGB on the device), as the other entries of metrics.METRICS.
    Keys: lpips_model ('vgg' | 'alexnet'); ours: lpips_weights | vgg16_path (alexnet_path) + lin_path, rgb (default false: the
    reference's BGR feed), normalize (default false: the reference's [0, 1] feed).  rgb + normalize is what the lpips package documents
    for RGB images in [0, 1].  The loaded weights and their plans are cached per backbone and resolved path."""
    paths = check_lpips_opt(lpips_model, **kw)
    net = _net(lpips_model)
    a, b = (t if t.dim() == 4 else t[None] for t in (img, img2))
    if a.shape[0] != 1:
        raise ValueError("one image per call (the reference validates with batch size 1)")
    key = (net,) + paths + (a.device.index,)
    if key not in _MODELS:
        _MODELS[key] = LPIPSModel(load_lpips_state(*paths, net=net), a.device, net=net)
    d = lpips_distance(a.contiguous(), b.contiguous(), _MODELS[key], bgr=not kw.get("rgb", False), normalize=bool(kw.get("normalize", False)))
    return float(d[0])
