"""VGG19 perceptual loss on MI355X: forward of the feature extractor on the generator output and on the target, feature-L1
losses, and the backward to the generator output — BasicSR's PerceptualLoss / VGGFeatureExtractor as configured by
/root/reference/ssr/options/esrgan_s2naip_urban.yml:123-137 and called at /root/reference/ssr/models/ssr_esrgan_model.py:153-160
(`l_g_percep, l_g_style = self.cri_perceptual(self.output, percep_gt)`).

VGG19 (torchvision `features`, frozen): 16 3x3 convolutions + ReLU, 2x2 max-pool after conv1_2 / conv2_2 / conv3_4 / conv4_4; the
loss reads the conv outputs BEFORE the ReLU.  The convolutions and their dgrads run on the conv kernels through the C ABI
(SSR_ACT_RELU epilogue, ReLU' masks); the tapped layers are exactly the ones in front of a pooling, so "ReLU + max-pool" is one
pass over the stored pre-ReLU feature (csrc/vgg.hip).  Only dgrads are needed (the extractor's parameters are frozen).
The layer table, the specs, the random weights and the forward's launches are cnn_backbone.py, shared with the LPIPS metric's VGG16
and AlexNet; what is here is the loss's own: option checks, normalisation, the Gram and L1 launches and the dgrad chain.
The gradient w.r.t. the generator output is ADDED to the L1-gradient buffer that the discriminator's input-gradient kernel
already folds in (train_step._phase_g), so no extra pass over the 128x128 output exists.

Style term (style_weight > 0, criterion 'l1'): per tapped layer the Gram matrices gram(F) = F^T F / (C*H*W) of the output's and the
target's features (csrc/gram.hip, fp32 [N, C, C]), l_g_style = style_weight * sum_k w_k * mean|gram(Fx) - gram(Ft)|, and its feature
gradient style_weight * w_k / (N*C^2) * 2/(C*H*W) * Fx sign(D) (D is symmetric) ADDED to the feature-L1 gradient of the layer before
the dgrad chain.  The target side gets no gradient (gt.detach()).  perceptual_weight 0 with a style term: BasicSR's feature term is
None, so the feature-L1 launches are skipped and only the style loss exists.

Weights: torchvision's checkpoint layout (`features.{idx}.weight/bias`, e.g. vgg19-dcbb9e9d.pth; BasicSR's `vgg_net.` prefix is
accepted too).  There is no network access here, so benchmarks and tests use random weights of the same architecture."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import torch

from . import cnn_backbone as CB, engine, hip
from .hip import view

VGG_PRETRAIN_PATH = "experiments/pretrained_models/vgg19-dcbb9e9d.pth"    # basicsr/archs/vgg_arch.py
VGG_MEAN = (0.485, 0.456, 0.406)
VGG_STD = (0.229, 0.224, 0.225)


def vgg19_layers():
    """[(name 'convB_J', torchvision features index, cin, cout, pooled_before)]"""
    return [(l.name, l.idx, l.cin, l.cout, bool(l.pool)) for l in CB.vgg_layers(CB.VGG19_BLOCKS)]


def vgg19_specs(last: str) -> List[engine.ConvSpec]:
    return CB.conv_specs(CB.vgg_layers(CB.VGG19_BLOCKS), last)


def vgg19_random_state(specs, seed: int = 0):
    """torchvision VGG._initialize_weights: kaiming_normal_(fan_out, relu), zero bias."""
    return CB.random_conv_state([(s.name, (s.cout, s.cin, s.k, s.k)) for s in specs], torch.Generator().manual_seed(seed))


def load_vgg19_state(path: str) -> Dict[str, torch.Tensor]:
    sd = CB.load_features_state(path)
    return {k[len("vgg_net."):] if k.startswith("vgg_net.") else k: v for k, v in sd.items() if "features." in k}


def check_perceptual_opt(opt: Dict) -> None:
    """The loss terms of `train.perceptual_opt` this library runs: criterion 'l1' for the feature and the style (Gram) terms."""
    if opt.get("type", "PerceptualLoss") != "PerceptualLoss":
        raise NotImplementedError(f"train.perceptual_opt.type={opt.get('type')!r}")
    if opt.get("vgg_type", "vgg19") != "vgg19":
        raise NotImplementedError(f"train.perceptual_opt.vgg_type={opt.get('vgg_type')!r}: only vgg19")
    if opt.get("criterion", "l1") != "l1":
        raise NotImplementedError(f"train.perceptual_opt.criterion={opt.get('criterion')!r}: only l1")
    if float(opt.get("style_weight", 0)) < 0.0:
        raise NotImplementedError(f"train.perceptual_opt.style_weight={opt.get('style_weight')!r}: BasicSR computes no style term below 0")


class PerceptualPlan:
    """Static launch lists for one (B, H, W): `fwd_target` (features of the target, no activations kept), `fwd` (features of
    the generator output, activations kept), `bwd` (loss, feature gradients, dgrads down to the image)."""

    def __init__(self, opt: Dict, B: int, H: int, W: int, dtype: int, x_buf: torch.Tensor, tgt_buf: torch.Tensor,
                 grad_buf: torch.Tensor, loss_ptr: int, num_ch: int = 3, state: Optional[Dict[str, torch.Tensor]] = None,
                 loss_flags: int = 0, style_loss_ptr: int = 0):
        check_perceptual_opt(opt)
        assert num_ch == 3 and H % 16 == 0 and W % 16 == 0, "VGG19 features need RGB images with H, W divisible by 16"
        self.layer_weights = {str(k): float(v) for k, v in opt["layer_weights"].items()}
        self.pw = float(opt.get("perceptual_weight", 1.0))
        self.sw = float(opt.get("style_weight", 0.0))
        self.style = self.sw > 0.0
        # BasicSR's feature term is None at perceptual_weight 0 - with a style term only (no style term: launched as before)
        self.feature = self.pw > 0.0 or not self.style
        if self.style and not style_loss_ptr:
            raise ValueError("PerceptualPlan: style_weight > 0 needs style_loss_ptr (the l_g_style slot)")
        net = CB.vgg_layers(CB.VGG19_BLOCKS)
        names = [l.name for l in net]
        for k in self.layer_weights:
            if k not in names:
                raise NotImplementedError(f"perceptual layer {k!r}: features are supported at conv outputs (before the ReLU)")
        last = max(self.layer_weights, key=names.index)
        net = net[:names.index(last) + 1]
        for l, nxt in zip(net, net[1:]):
            # a tapped layer is stored before its ReLU; the fused ReLU+pool pass needs a pooling behind it
            if l.name in self.layer_weights and not nxt.pool:
                raise NotImplementedError(f"perceptual layer {l.name!r}: taps are supported in front of a pooling layer (and at the last layer)")
        mode = dtype                          # (hip.F32F: the VGG forward in exact fp32 too - its ReLU decisions shape the image gradient)
        dtype = hip.storage_code(mode)
        self.dt, self.B, self.H, self.W = dtype, B, H, W
        tdt = hip.torch_dtype(dtype)
        dev = x_buf.device
        self.store = engine.ParamStore(CB.conv_specs(net), mode, device=dev)
        sd = state
        self.random_weights = False
        if sd is None:
            # BasicSR's VGGFeatureExtractor: experiments/pretrained_models/vgg19-dcbb9e9d.pth if present, else torchvision's
            # download.  There is no download here: the file (torchvision layout) must exist, or the caller passes `state`.
            cands = [opt.get("pretrained_path"), os.environ.get("SSR_VGG19_WEIGHTS"), VGG_PRETRAIN_PATH]
            path = next((c for c in cands if c and os.path.exists(c)), None)
            if path is not None:
                sd = load_vgg19_state(path)
            elif os.environ.get("SSR_VGG19_RANDOM") == "1":   # explicit opt-in: throughput runs without the published weights
                sd = vgg19_random_state(list(self.store.specs.values()), seed=int(opt.get("seed", 0)))
                self.random_weights = True
            else:
                raise FileNotFoundError(
                    f"perceptual_opt needs the VGG19 weights: put torchvision's vgg19-dcbb9e9d.pth at {VGG_PRETRAIN_PATH} (BasicSR's "
                    "location), or set SSR_VGG19_WEIGHTS=<file>; SSR_VGG19_RANDOM=1 runs with random weights (throughput only)")
        self.store.load_state_dict(sd)
        z = lambda *s: torch.zeros(B, *s, dtype=tdt, device=dev)
        use_norm, range_norm = bool(opt.get("use_input_norm", True)), bool(opt.get("range_norm", False))
        # y = ((x + 1)/2 if range_norm else x - mean)/std ...   as one per-channel affine map
        a = 0.5 if range_norm else 1.0
        b = 0.5 if range_norm else 0.0
        mean, std = (VGG_MEAN, VGG_STD) if use_norm else ((0.0,) * 3, (1.0,) * 3)
        self._scale = (C.c_float * 8)(*[a / s for s in std], *([0.0] * 5))
        self._shift = (C.c_float * 8)(*[(b - m) / s for m, s in zip(mean, std)], *([0.0] * 5))
        self._zero = (C.c_float * 8)(*([0.0] * 8))
        self.xn = z(H, W, 8)             # normalised image (3 of 8 channels)
        self.g_xn = z(H, W, 8)
        cb = engine._ConvBuilder(self.store, B)
        self._cb = cb
        lib = hip.lib()
        # activations: per conv either the post-ReLU output (plain layers) or the pre-ReLU feature (tapped layers) + its pooled twin
        acts, pooled = CB.forward_buffers(net, H, W, z, self.layer_weights, True)
        g_acts, g_pooled = CB.forward_buffers(net, H, W, z, self.layer_weights, True)
        feats_t = {name: torch.zeros_like(acts[name]) for name in acts if name in self.layer_weights}
        dims = dict(zip(names, CB.tap_sizes(net, H, W)))
        layers = vgg19_layers()[:len(net)]           # as `layers` exposes them: (name, index, cin, cout, pooled_before)
        self.acts, self.feats_t, self.g_acts = acts, feats_t, g_acts
        npix = B * H * W

        def forward(img: torch.Tensor, outs: Dict[str, torch.Tensor]) -> engine.Launcher:
            L = engine.Launcher()
            L.add(lib.ssr_channel_affine, view(img), view(self.xn), dtype, npix, 3, self._scale, self._shift, 0, what="vgg normalise")
            CB.append_forward(L, cb, lib, net, self.xn, H, W, B, dtype, self.layer_weights,
                              lambda name: outs[name] if name in self.layer_weights else acts[name], pooled, True)
            return L

        self.fwd_target = forward(tgt_buf, feats_t)
        self.fwd = forward(x_buf, acts)
        # ---- style term: Gram matrices of the target's features (fwd_target) and of the output's (fwd), then |D| and sign(D)
        self.gram_x, self.gram_t, self.gram_s = {}, {}, {}
        if self.style:
            splits = {}
            for name in self.layer_weights:
                hh, ww = dims[name]
                cout = acts[name].shape[-1]
                splits[name] = lib.ssr_gram_splits(B, hh * ww, cout)
                hip.check(min(splits[name], 0), f"ssr_gram_splits {name}")
                self.gram_x[name] = torch.zeros(B, cout, cout, dtype=torch.float32, device=dev)
                self.gram_t[name] = torch.zeros(B, cout, cout, dtype=torch.float32, device=dev)
                self.gram_s[name] = z(cout, cout)          # sign(D) in the feature dtype (+-1 / 0: exact)
            # one split-partial workspace for every Gram launch (they run in order on one stream)
            ws_n = max([splits[k] * B * acts[k].shape[-1] ** 2 for k in splits if splits[k] > 1] or [1])
            self.gram_ws = torch.zeros(ws_n, dtype=torch.float32, device=dev)
            for name, wgt in self.layer_weights.items():
                hh, ww = dims[name]
                cout = acts[name].shape[-1]
                gscale = 1.0 / (cout * hh * ww)
                self.fwd_target.add(lib.ssr_gram_fwd, view(feats_t[name]), self.gram_t[name].data_ptr(), self.gram_ws.data_ptr(), dtype, B,
                                    hh * ww, cout, gscale, what=f"gram target {name}")
                self.fwd.add(lib.ssr_gram_fwd, view(acts[name]), self.gram_x[name].data_ptr(), self.gram_ws.data_ptr(), dtype, B, hh * ww,
                             cout, gscale, what=f"gram {name}")
                # l_g_style += sw * w_k * mean|Gx - Gt|
                self.fwd.add(lib.ssr_gram_l1, self.gram_x[name].data_ptr(), self.gram_t[name].data_ptr(), self.gram_s[name].data_ptr(),
                             dtype | loss_flags, B * cout * cout, self.sw * wgt / (B * cout * cout), style_loss_ptr, what=f"gram L1 {name}")
        # ---- backward: losses + feature gradients, then dgrads from the last layer down to the image
        Bk = engine.Launcher()
        for name, wgt in self.layer_weights.items():
            hh, ww = dims[name]
            cout = acts[name].shape[-1]
            # loss += w_k * pw * mean|Fx - Ft| ; g_F = w_k * pw * sign(Fx - Ft) / numel
            if self.feature:
                Bk.add(lib.ssr_l1_loss, view(acts[name]), view(feats_t[name]), view(g_acts[name]), dtype | loss_flags, B * hh * ww, cout,
                       wgt * self.pw, loss_ptr, what=f"feature L1 {name}")
            if self.style:
                # g_F (+)= sw * w_k / (N C^2) * 2 / (C H W) * Fx sign(D)
                coef = self.sw * wgt / (B * cout * cout) * 2.0 / (cout * hh * ww)
                Bk.add(lib.ssr_gram_bwd, view(acts[name]), self.gram_s[name].data_ptr(), view(g_acts[name]), dtype, B, hh * ww, cout, coef,
                       1 if self.feature else 0, what=f"gram bwd {name}")
        for li in reversed(range(len(net))):
            name, idx, cout = net[li].name, net[li].idx, net[li].cout
            hh, ww = dims[name]
            if li == 0:      # conv1_1: gradient w.r.t. the normalised image (3 channels), no mask
                cb.dgrad(Bk, f"features.{idx}", view(g_acts[name]), hh, ww, view(self.g_xn), cout=8, cin_dy=cout)
                break
            pname = net[li - 1].name
            if net[li].pool:
                # input is pooled[pname]: plain dgrad into its gradient, then route through ReLU + pooling into the tapped feature
                cb.dgrad(Bk, f"features.{idx}", view(g_acts[name]), hh, ww, view(g_pooled[pname]))
                ph, pw_ = dims[pname]
                Bk.add(lib.ssr_relu_maxpool2_bwd, view(acts[pname]), view(g_pooled[pname]), view(g_acts[pname]), dtype, B, ph, pw_,
                       acts[pname].shape[-1], 1, what=f"relu+pool bwd {pname}")
            else:
                # input is the ReLU output of a plain layer: ReLU' from the sign of the stored activation
                assert pname not in self.layer_weights
                cb.dgrad(Bk, f"features.{idx}", view(g_acts[name]), hh, ww, view(g_acts[pname]), m=view(acts[pname]), m_c0=0,
                         m_c1=acts[pname].shape[-1], m_relu=1)
        # d loss / d image = d loss / d xn * scale, added to the generator's output-gradient residual
        self._gscale = (C.c_float * 8)(*[float(self._scale[c]) for c in range(3)], *([0.0] * 5))
        Bk.add(lib.ssr_channel_affine, view(self.g_xn), view(grad_buf), dtype, npix, 3, self._gscale, self._zero, 1, what="vgg normalise bwd")
        self.bwd = Bk
        self.layers, self.dims, self.pooled, self.g_pooled = layers, dims, pooled, g_pooled

    def pack(self):
        self.store.pack()
