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

    vgg16_layers / vgg16_specs     the layer table
    load_lpips_state               torchvision + lpips files, one lpips state_dict, or the flat layout -> flat layout
    lpips_random_state             random weights of the same architecture (tests, throughput runs)
    lpips_reference                the definition in torch on the CPU
    LPIPSPlan / LPIPSModel         the static launch list for one (N, H, W) / the weights on the device and their plans
    lpips_distance                 uint8 NHWC device images -> float64 [N] on the host
    calculate_lpips                the entry of metrics.METRICS
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

LPIPS_PRETRAIN_PATH = "experiments/pretrained_models/lpips_vgg.pth"
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
LPIPS_EPS = 1e-10
# (block, convs in the block, width)
VGG16_BLOCKS = ((1, 2, 64), (2, 2, 128), (3, 3, 256), (4, 3, 512), (5, 3, 512))
LPIPS_TAPS = ("conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3")
# keys of a `calculate_lpips` metric entry: the reference's **kwargs swallows the first four
_IGNORED_KEYS = ("crop_border", "test_y_channel", "input_order", "better", "type")
_OUR_KEYS = ("lpips_model", "lpips_weights", "vgg16_path", "lin_path", "rgb", "normalize")


def vgg16_layers():
    """[(name 'convB_J', torchvision features index, cin, cout, pooled_before)]"""
    out, idx, cin = [], 0, 3
    for b, n, width in VGG16_BLOCKS:
        for j in range(1, n + 1):
            out.append((f"conv{b}_{j}", idx, cin, width, j == 1 and b > 1))
            idx += 2                    # conv, relu
            cin = width
        idx += 1                        # pool
    return out


def vgg16_specs():
    from . import engine
    # no backward here: the transposed packing of the weights is left out
    return [engine.ConvSpec(f"features.{idx}", cout, cin, 3, 1, True, False, dgrad_packed=False) for _, idx, cin, cout, _ in vgg16_layers()]


def _tap_widths() -> List[int]:
    width = {n: cout for n, _, _, cout, _ in vgg16_layers()}
    return [width[t] for t in LPIPS_TAPS]


def lpips_random_state(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Flat layout.  Convolutions as torchvision's VGG._initialize_weights (kaiming_normal_(fan_out, relu), zero bias), `lin`
    weights from U[0, 1) (the package's are non-negative: the metric is a weighted sum of squares)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for _, idx, cin, cout, _ in vgg16_layers():
        sd[f"features.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (cout * 9))
        sd[f"features.{idx}.bias"] = torch.zeros(cout)
    for k, c in enumerate(_tap_widths()):
        sd[f"lin{k}"] = torch.rand(c, generator=g)
    return sd


def _torch_load(path: str) -> Dict[str, torch.Tensor]:
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return sd


def load_lpips_state(backbone_path: str, lin_path: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """-> {features.{idx}.weight / .bias (13 convolutions), lin{k} [C_k] (5 taps)}, float32, from any of   [recalled]
      * torchvision's vgg16-397923af.pth (`features.{idx}.*`) + the lpips package's weights/v0.1/vgg.pth (`lin{k}.model.1.weight`);
      * one file saved from lpips.LPIPS(net='vgg').state_dict(): `net.slice{s}.{idx}.*` with the same torchvision indices and
        `lin{k}.model.1.weight` (the duplicate `lins.{k}.*` and the `scaling_layer.*` keys are ignored);
      * the flat layout itself.
    KeyError / ValueError name the key that is missing / mis-shaped."""
    sd = dict(_torch_load(backbone_path))
    lin_sd = _torch_load(lin_path) if lin_path else {}
    out = {}
    for _, idx, cin, cout, _ in vgg16_layers():
        for leaf, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"features.{idx}.{leaf}"
            cands = [key] + [f"net.slice{s}.{idx}.{leaf}" for s in range(1, 6)]
            src = next((c for c in cands if c in sd), None)
            if src is None:
                raise KeyError(f"{key} (or net.slice{{s}}.{idx}.{leaf}) not in {backbone_path}")
            t = sd[src]
            if tuple(t.shape) != shape:
                raise ValueError(f"{src}: shape {tuple(t.shape)}, expected {shape}")
            out[key] = t.detach().to(torch.float32).clone()
    for k, c in enumerate(_tap_widths()):
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


def vgg16_tap_features(x: torch.Tensor, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the five post-ReLU taps of an NCHW input"""
    feats = {}
    for name, idx, _, _, pooled_before in vgg16_layers():
        if pooled_before:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, state[f"features.{idx}.weight"].to(x.dtype), state[f"features.{idx}.bias"].to(x.dtype), padding=1))
        if name in LPIPS_TAPS:
            feats[name] = x
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
                    dtype=torch.float64) -> torch.Tensor:
    """LPIPS(net='vgg', version='0.1') of uint8 [N, H, W, 3] RGB image pairs as the reference feeds it (module docstring) -> [N]"""
    with torch.no_grad():
        f0 = vgg16_tap_features(lpips_scaled_input(a_u8, bgr, normalize, dtype), state)
        f1 = vgg16_tap_features(lpips_scaled_input(b_u8, bgr, normalize, dtype), state)
        return lpips_from_features(f0, f1, {t: state[f"lin{k}"] for k, t in enumerate(LPIPS_TAPS)})


# ---------------------------------------------------------------- the device path
class LPIPSPlan:
    """One static launch list for N image pairs of H x W: ssr_lpips_input for both images (one batch of 2N), the 13 convolutions
    with the ReLU epilogue (the tapped ones stored before their ReLU), ssr_relu_maxpool2_fwd behind taps 1-4, five ssr_lpips_layer.
    The ParamStore is the exact fp32 mode's; `store` shares one (already loaded and packed) between the plans of a LPIPSModel."""

    def __init__(self, N: int, H: int, W: int, state: Optional[Dict[str, torch.Tensor]], device="cuda", bgr: bool = True,
                 normalize: bool = False, store=None, lins: Optional[torch.Tensor] = None):
        from . import engine, hip
        from .hip import view
        if N <= 0 or H <= 0 or W <= 0 or H % 16 or W % 16:
            raise ValueError(f"LPIPS (VGG16, four poolings) needs H and W divisible by 16, got {N} x {H} x {W}")
        dev = torch.device(device)
        self.N, self.H, self.W = N, H, W
        if store is None:
            store, lins = _device_weights(state, dev)
        self.store, self.lins = store, lins
        lib = hip.lib()
        B = 2 * N
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)      # noqa: E731
        self.a_u8 = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
        self.b_u8 = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
        self.xn = z(B, H, W, 8)
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
        layers = vgg16_layers()
        self.acts, self.pooled, taps = {}, {}, []
        src, h, w = self.xn, H, W
        for name, idx, cin, cout, pooled_before in layers:
            if pooled_before:
                h, w = h // 2, w // 2
            dst = self.acts[name] = z(B, h, w, cout)
            tapped = name in LPIPS_TAPS
            cb.conv(L, f"features.{idx}", view(src), h, w, view(dst), act=hip.ACT_NONE if tapped else hip.ACT_RELU)
            src = dst
            if tapped:
                taps.append((name, h * w, cout))
                if name != LPIPS_TAPS[-1]:
                    self.pooled[name] = z(B, h // 2, w // 2, cout)
                    L.add(lib.ssr_relu_maxpool2_fwd, view(dst), view(self.pooled[name]), hip.F32, B, h, w, cout, what=f"relu+pool {name}")
                    src = self.pooled[name]
        # partials: per tap [N][nblk] doubles, one buffer, one download
        self.slices, off, woff = [], 0, 0
        for name, hw, c in taps:
            nblk = lib.ssr_lpips_layer_blocks(N, hw, c)
            hip.check(min(nblk, 0), f"ssr_lpips_layer_blocks {name}")
            self.slices.append((off, nblk))
            off += N * nblk
        self.partial = torch.zeros(off, dtype=torch.float64, device=dev)
        for (name, hw, c), (poff, nblk) in zip(taps, self.slices):
            f = self.acts[name]
            L.add(lib.ssr_lpips_layer, view(f[:N]), view(f[N:]), self.lins.data_ptr() + 4 * woff, hip.F32, N, hw, c, 1,
                  self.partial.data_ptr() + 8 * poff, what=f"lpips layer {name}")
            woff += c
        self.launcher = L

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


def _device_weights(state: Dict[str, torch.Tensor], dev):
    """(ParamStore of the VGG16 convolutions in the exact fp32 mode, loaded and packed; the five lin vectors as one fp32 tensor)"""
    from . import engine, hip
    widths = _tap_widths()
    for k, c in enumerate(widths):
        if f"lin{k}" not in state:
            raise KeyError(f"lin{k}")
        if tuple(state[f"lin{k}"].shape) != (c,):
            raise ValueError(f"lin{k}: shape {tuple(state[f'lin{k}'].shape)}, expected ({c},)")
    store = engine.ParamStore(vgg16_specs(), hip.F32, device=dev)
    store.load_state_dict(state)
    store.pack()
    lins = torch.cat([state[f"lin{k}"].to(torch.float32) for k in range(len(widths))]).to(dev)
    return store, lins


class LPIPSModel:
    """The weights on the device and the plans that use them, cached per (N, H, W, bgr, normalize)."""

    def __init__(self, state: Dict[str, torch.Tensor], device="cuda"):
        self.device = torch.device(device)
        self.store, self.lins = _device_weights(state, self.device)
        self.plans: Dict[Tuple, LPIPSPlan] = {}

    def plan(self, N: int, H: int, W: int, bgr: bool = True, normalize: bool = False) -> LPIPSPlan:
        key = (N, H, W, bool(bgr), bool(normalize))
        if key not in self.plans:
            self.plans[key] = LPIPSPlan(N, H, W, None, self.device, bgr=bgr, normalize=normalize, store=self.store, lins=self.lins)
        return self.plans[key]


def lpips_distance(a_u8: torch.Tensor, b_u8: torch.Tensor, model: LPIPSModel, bgr: bool = True, normalize: bool = False) -> torch.Tensor:
    """a_u8, b_u8: uint8 [N, H, W, 3] RGB device tensors as `tensor2img_u8` gives them -> float64 [N] on the host."""
    if not (a_u8.shape == b_u8.shape and a_u8.dtype == torch.uint8 and b_u8.dtype == torch.uint8 and a_u8.is_cuda and b_u8.is_cuda):
        raise ValueError(f"Image shapes are different: {tuple(a_u8.shape)}, {tuple(b_u8.shape)} (uint8 device tensors)")
    if a_u8.dim() != 4 or a_u8.shape[-1] != 3:
        raise ValueError(f"LPIPS needs uint8 [N, H, W, 3] images, got {tuple(a_u8.shape)}")
    n, h, w, _ = a_u8.shape
    return model.plan(n, h, w, bgr, normalize).run(a_u8, b_u8)


# ---------------------------------------------------------------- the metric entry
_MODELS: Dict[Tuple, LPIPSModel] = {}


def check_lpips_opt(lpips_model="vgg", **kw) -> Tuple[str, Optional[str]]:
    """Validates the keys of a `calculate_lpips` entry and finds the weights -> (backbone or combined file, lin file or None).
    Touches no device: the model plugin calls it before the first validation image is processed."""
    if lpips_model != "vgg":
        raise NotImplementedError(f"metric type 'calculate_lpips': lpips_model={lpips_model!r}: only 'vgg' (alexnet needs 11x11 stride-4 "
                                  "and 5x5 convolutions and 3x3 stride-2 pooling; no shipped option file asks for it)")
    for k in kw:
        if k not in _IGNORED_KEYS and k not in _OUR_KEYS:
            raise NotImplementedError(f"metric type 'calculate_lpips': option {k!r} (have {sorted(_OUR_KEYS)})")
    combined, vgg, lin = kw.get("lpips_weights"), kw.get("vgg16_path"), kw.get("lin_path")
    if combined and (vgg or lin):
        raise ValueError("metric type 'calculate_lpips': give lpips_weights (one combined file) or vgg16_path + lin_path, not both")
    if bool(vgg) != bool(lin):
        raise ValueError("metric type 'calculate_lpips': vgg16_path and lin_path go together (the backbone and the lpips package's linear layers)")
    for key, path in (("lpips_weights", combined), ("vgg16_path", vgg), ("lin_path", lin)):
        if path and not os.path.exists(path):
            raise FileNotFoundError(f"metric type 'calculate_lpips': {key}={path!r} does not exist")
    if combined:
        return os.path.abspath(combined), None
    if vgg:
        return os.path.abspath(vgg), os.path.abspath(lin)
    for cand in (os.environ.get("SSR_LPIPS_WEIGHTS"), LPIPS_PRETRAIN_PATH):
        if cand and os.path.exists(cand):
            return os.path.abspath(cand), None
    raise NotImplementedError(
        "metric type 'calculate_lpips': no LPIPS weights found.  Put them in one of three places: the metric's options (`lpips_weights: "
        "<file saved from lpips.LPIPS(net='vgg').state_dict()>`, or `vgg16_path: <torchvision vgg16-397923af.pth>` + `lin_path: <lpips "
        f"weights/v0.1/vgg.pth>`), the environment variable SSR_LPIPS_WEIGHTS=<combined file>, or {LPIPS_PRETRAIN_PATH}.  "
        "There is no silent random network: a metric from random weights is not LPIPS")


def calculate_lpips(img, img2, lpips_model="vgg", **kw) -> float:
    """One image pair per call (uint8 [1, H, W, 3] or [H, W, 3] RGB on the device), as the other entries of metrics.METRICS.
    Keys: lpips_model ('vgg'); ours: lpips_weights | vgg16_path + lin_path, rgb (default false: the reference's BGR feed),
    normalize (default false: the reference's [0, 1] feed).  rgb + normalize is what the lpips package documents for RGB images in
    [0, 1].  The loaded weights and their plans are cached per resolved path."""
    paths = check_lpips_opt(lpips_model, **kw)
    a, b = (t if t.dim() == 4 else t[None] for t in (img, img2))
    if a.shape[0] != 1:
        raise ValueError("one image per call (the reference validates with batch size 1)")
    key = paths + (a.device.index,)
    if key not in _MODELS:
        _MODELS[key] = LPIPSModel(load_lpips_state(*paths), a.device)
    d = lpips_distance(a.contiguous(), b.contiguous(), _MODELS[key], bgr=not kw.get("rgb", False), normalize=bool(kw.get("normalize", False)))
    return float(d[0])
