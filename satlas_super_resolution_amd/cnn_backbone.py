"""The torchvision-style CNN feature extractors, written once: VGG19 (the perceptual and style loss, perceptual.py), VGG16 and AlexNet
(the LPIPS metric, lpips_metric.py).  One layer record, one geometry walk, one ConvSpec list, one random state per initialisation,
one file loader and one forward emitter; the loss and the metric keep what is their own (normalisation, taps, Gram / L1 / lpips
launches, the dgrad chain).

    Layer                      name, torchvision `features` index, cin, cout, kernel, stride, pad, the pooling in front
    vgg_layers(blocks)         the VGG tables from VGG16_BLOCKS / VGG19_BLOCKS;  ALEXNET_LAYERS: the same record, written out
    tap_sizes                  (h, w) of every layer's output for an H x W image
    conv_specs                 the 3 x 3 layers, which ssr_conv2d runs, as ParamStore specs
    conv_shapes / random_conv_state / load_features_state      the weights: shapes, random ones, a torchvision file
    forward_buffers / append_forward                           the activations and the launches of one forward

A forward is: where the record has a 3 x 3 stride-2 pooling in front, ssr_maxpool3s2_fwd; the convolution with the ReLU epilogue,
through ssr_conv2d (3 x 3) or ssr_conv_direct (any other kernel, and a 3 x 3 layer whose grid ssr_conv2d refuses); a layer tapped
before its ReLU is stored without it and, unless it is the last, followed by ssr_relu_maxpool2_fwd - such taps sit in front of a
2 x 2 pooling, which is how that pooling is run and the only way it is."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from . import engine, hip
from .hip import view


class Layer(NamedTuple):
    name: str
    idx: int            # position in torchvision's `features`
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    pool: int           # the pooling in front: 0 none, 2 = 2x2 stride 2, 3 = 3x3 stride 2 (no padding, floor mode)


# (block, convs in the block, width)
VGG16_BLOCKS = ((1, 2, 64), (2, 2, 128), (3, 3, 256), (4, 3, 512), (5, 3, 512))
VGG19_BLOCKS = ((1, 2, 64), (2, 2, 128), (3, 4, 256), (4, 4, 512), (5, 4, 512))
ALEXNET_LAYERS = (Layer("conv1", 0, 3, 64, 11, 4, 2, 0), Layer("conv2", 3, 64, 192, 5, 1, 2, 3), Layer("conv3", 6, 192, 384, 3, 1, 1, 3),
                  Layer("conv4", 8, 384, 256, 3, 1, 1, 0), Layer("conv5", 10, 256, 256, 3, 1, 1, 0))                      # [recalled]


def vgg_layers(blocks) -> List[Layer]:
    """'convB_J': 3x3 convolutions + ReLU, a 2x2 pooling between the blocks"""
    out, idx, cin = [], 0, 3
    for b, n, width in blocks:
        for j in range(1, n + 1):
            out.append(Layer(f"conv{b}_{j}", idx, cin, width, 3, 1, 1, 2 if j == 1 and b > 1 else 0))
            idx += 2                    # conv, relu
            cin = width
        idx += 1                        # pool
    return out


def tap_sizes(layers, H: int, W: int) -> List[Tuple[int, int]]:
    out, h, w = [], H, W
    for l in layers:
        if l.pool:
            h, w = (h - l.pool) // 2 + 1, (w - l.pool) // 2 + 1
        h, w = (h + 2 * l.pad - l.k) // l.stride + 1, (w + 2 * l.pad - l.k) // l.stride + 1
        out.append((h, w))
    return out


def conv_specs(layers, last: Optional[str] = None, dgrad_packed: bool = True) -> List[engine.ConvSpec]:
    """the 3 x 3 layers up to and including `last`; dgrad_packed=False where no backward runs: the transposed packing is left out"""
    specs = []
    for l in layers:
        if l.k == 3:
            specs.append(engine.ConvSpec(f"features.{l.idx}", l.cout, l.cin, 3, 1, True, False, dgrad_packed=dgrad_packed))
        if l.name == last:
            break
    return specs


def conv_shapes(layers) -> List[Tuple[str, Tuple[int, int, int, int]]]:
    """[(torchvision key 'features.{idx}', weight shape)]"""
    return [(f"features.{l.idx}", (l.cout, l.cin, l.k, l.k)) for l in layers]


def random_conv_state(shapes, g: torch.Generator, kaiming: bool = True) -> Dict[str, torch.Tensor]:
    """kaiming: torchvision's VGG._initialize_weights, kaiming_normal_(fan_out, relu) and zero bias.  Otherwise nn.Conv2d's default,
    which torchvision's AlexNet keeps: weights and biases from U(-b, b), b = 1 / sqrt(fan_in) [recalled].  One draw per tensor from `g`,
    in the order of `shapes`, weight before bias."""
    sd = {}
    for key, (cout, cin, kh, kw) in shapes:
        if kaiming:
            sd[key + ".weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cout * kh * kw))
            sd[key + ".bias"] = torch.zeros(cout)
        else:
            b = 1.0 / math.sqrt(cin * kh * kw)
            sd[key + ".weight"] = (2 * torch.rand(cout, cin, kh, kw, generator=g) - 1) * b
            sd[key + ".bias"] = (2 * torch.rand(cout, generator=g) - 1) * b
    return sd


def load_features_state(path: str) -> Dict[str, torch.Tensor]:
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: not a state_dict")
    return sd


def forward_buffers(layers, H: int, W: int, z: Callable, tapped, tap_pre_relu: bool):
    """-> (acts {layer: z(h, w, cout)}, pooled): the output of every layer and of every pooling, the latter under the name of the
    layer behind a 3x3 pooling, and of the tap in front of a 2x2 one (no other 2x2 pooling is run)"""
    acts, pooled, h, w = {}, {}, H, W
    for i, (l, (ho, wo)) in enumerate(zip(layers, tap_sizes(layers, H, W))):
        if l.pool == 3:
            pooled[l.name] = z((h - 3) // 2 + 1, (w - 3) // 2 + 1, l.cin)
        acts[l.name] = z(ho, wo, l.cout)
        if tap_pre_relu and l.name in tapped and i + 1 < len(layers):
            pooled[l.name] = z(ho // 2, wo // 2, l.cout)
        h, w = ho, wo
    return acts, pooled


def append_forward(L: engine.Launcher, cb: engine._ConvBuilder, lib, layers, src: torch.Tensor, H: int, W: int, B: int, dtype: int,
                   tapped, dst_of: Callable, pooled: Dict[str, torch.Tensor], tap_pre_relu: bool, direct=None):
    """Appends the forward of `layers` over `src` ([B, H, W, 8]) to L.  dst_of(name): where a layer's output goes; `pooled` as
    forward_buffers names it; tap_pre_relu: the `tapped` layers are stored before their ReLU.  `direct`: {layer: (weights
    [K*K][CinPad][Cout], bias)} for ssr_conv_direct; where it is given, ssr_conv2d_variant is asked once per 3 x 3 layer (a question
    of the shape, never of the batch) and SSR_EUNSUP sends the layer to ssr_conv_direct.
    -> ([(h, w)] per layer, [(name, h * w, cout)] per tapped layer)"""
    sizes, taps, h, w = tap_sizes(layers, H, W), [], H, W
    for i, (l, (ho, wo)) in enumerate(zip(layers, sizes)):
        if l.pool == 3:
            p = pooled[l.name]
            L.add(lib.ssr_maxpool3s2_fwd, view(src), view(p), dtype, B, h, w, l.cin, 0, what=f"pool in front of {l.name}")
            src = p
        if l.pool:
            h, w = (h - l.pool) // 2 + 1, (w - l.pool) // 2 + 1
        dst, tap = dst_of(l.name), l.name in tapped
        use_direct = l.k != 3
        if not use_direct:
            cb.conv(L, f"features.{l.idx}", view(src), h, w, view(dst), act=hip.ACT_NONE if tap and tap_pre_relu else hip.ACT_RELU)
            rc = lib.ssr_conv2d_variant(C.byref(cb.keep[-1])) if direct else 0
            if rc == -2:                              # SSR_EUNSUP for this grid: the generic kernel
                L.calls.pop()
                use_direct = True
            elif rc < 0:
                hip.check(rc, f"ssr_conv2d_variant {l.name}")
        if use_direct:
            wd, bd = direct[l.name]
            L.add(lib.ssr_conv_direct, view(src), view(dst), wd.data_ptr(), bd.data_ptr(), dtype, B, h, w, wd.shape[1], l.cout, l.k,
                  l.stride, l.pad, 1, what=f"conv direct {l.name}")
        src, h, w = dst, ho, wo
        if tap:
            taps.append((l.name, ho * wo, l.cout))
            if tap_pre_relu and i + 1 < len(layers):
                L.add(lib.ssr_relu_maxpool2_fwd, view(dst), view(pooled[l.name]), dtype, B, ho, wo, l.cout, what=f"relu+pool {l.name}")
                src = pooled[l.name]
    return sizes, taps
