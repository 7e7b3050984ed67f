"""OSMObjDiscriminator on MI355X - same registry name, constructor, forward contract and state_dict layout as
/root/reference/ssr/archs/osm_obj_discriminator_arch.py:34-108.

forward(x: float32[B, num_in_ch, H, W], osm_objs: float32[Bo, 3, Ho, Wo]) -> (out: float32[B, 1, H, W], o_out: float32[Bo, 1, Ho / 16,
Wo / 16]).  The U-Net half (:82-107) is layer for layer SSR_UNetDiscriminatorSN and runs through the same engine.DiscriminatorPlan in
the network's arithmetic mode; the object branch (:74-79: four biased 4x4 stride-2 convolutions with ReLU, two SelfAttentionBlocks)
runs through engine.ObjectBranchPlan in exact fp32 in every mode.  Ho, Wo in {16, 32}: 32 x 32 is what the reference's model feeds
(osm_objs_esrgan_model.py resizes every crop to it).

state_dict: the reference's 50 keys in its order - o_conv1, o_conv2, o_attention1.{gamma, query_conv, key_conv, value_conv}, o_conv3,
o_attention2.*, o_conv4 (weight + bias each), then conv0 .. conv9 as SSR_UNetDiscriminatorSN holds them."""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

from .. import engine, hip
from ..registry import ARCH_REGISTRY
from .hipnet import ConvParams, HipNet


class _AttentionParams(nn.Module):
    """Parameter holder of one SelfAttentionBlock (osm_obj_discriminator_arch.py:9-14; never called)."""

    def __init__(self, channels: int):
        super().__init__()
        self.query_conv = ConvParams(engine.ConvSpec("query_conv", channels // 8, channels, 1, 1), "default")
        self.key_conv = ConvParams(engine.ConvSpec("key_conv", channels // 8, channels, 1, 1), "default")
        self.value_conv = ConvParams(engine.ConvSpec("value_conv", channels, channels, 1, 1), "default")
        self.gamma = nn.Parameter(torch.zeros(1))


class _OSMDiscriminatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, osm_objs, *params):
        st = net.store()
        ost = net._ostore
        lib = hip.lib()
        B, C, H, W = x.shape
        Bo, Co, Ho, Wo = osm_objs.shape
        plan, xin = net.plan(B, H, W)
        oplan = net.object_plan(Bo, Ho, Wo)
        st.spectral_norm(power_iter=net.training)
        st.pack()
        ost.pack()
        xc = x.detach().contiguous().float()
        hip.check(lib.ssr_nchw_to_nhwc(xc.data_ptr(), B, C, H, W, hip.view(xin), st.dtype, 1, 1, 1.0, hip.stream_ptr()), "ssr_nchw_to_nhwc")
        oc = osm_objs.detach().contiguous().float()
        hip.check(lib.ssr_nchw_to_nhwc(oc.data_ptr(), Bo, Co, Ho, Wo, hip.view(oplan.xin), hip.F32, 1, 1, 1.0, hip.stream_ptr()),
                  "ssr_nchw_to_nhwc")
        plan.forward_plan(xin).run()
        oplan.fwd.run()
        plan.generation = getattr(plan, "generation", 0) + 1
        oplan.generation = getattr(oplan, "generation", 0) + 1
        ctx.net, ctx.plan, ctx.xin, ctx.oplan, ctx.gen = net, plan, xin, oplan, (plan.generation, oplan.generation)
        out = torch.empty(B, 1, H, W, device=x.device)
        hip.check(lib.ssr_nhwc_to_nchw(hip.view(plan.logits), st.dtype, out.data_ptr(), B, 1, H, W, hip.stream_ptr()), "ssr_nhwc_to_nchw")
        o_out = torch.empty(Bo, 1, Ho // 16, Wo // 16, device=x.device)
        hip.check(lib.ssr_nhwc_to_nchw(hip.view(oplan.out), hip.F32, o_out.data_ptr(), Bo, 1, Ho // 16, Wo // 16, hip.stream_ptr()),
                  "ssr_nhwc_to_nchw")
        return out, o_out

    @staticmethod
    def backward(ctx, gy, go):
        net, plan, xin, oplan = ctx.net, ctx.plan, ctx.xin, ctx.oplan
        if (plan.generation, oplan.generation) != ctx.gen:
            raise RuntimeError("OSMObjDiscriminator: activations of this forward were overwritten by a later forward; call "
                               "backward() before the next forward (as the reference loop does)")
        st = net.store()
        ost = net._ostore
        lib = hip.lib()
        B, _, H, W = gy.shape
        Bo, _, ho, wo = go.shape
        g = gy.contiguous().float()
        hip.check(lib.ssr_nchw_to_nhwc(g.data_ptr(), B, 1, H, W, hip.view(plan.d_logits), st.dtype, 1, 1, 1.0, hip.stream_ptr()),
                  "ssr_nchw_to_nhwc")
        g2 = go.contiguous().float()
        hip.check(lib.ssr_nchw_to_nhwc(g2.data_ptr(), Bo, 1, ho, wo, hip.view(oplan.d_out), hip.F32, 1, 1, 1.0, hip.stream_ptr()),
                  "ssr_nchw_to_nhwc")
        needs = list(ctx.needs_input_grad[3:])
        pg, ig, iog = any(needs), ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        st.grad.zero_()
        st.grad_sn.zero_()
        ost.grad.zero_()
        plan.backward_plan(xin, param_grads=pg, input_grad=ig).run()
        oplan.backward_plan(param_grads=pg, input_grad=iog).run()
        if pg:
            st.spectral_norm_backward()
        gx = gosm = None
        if ig:
            gx = torch.empty(B, net.num_in_ch, H, W, device=gy.device)
            hip.check(lib.ssr_nhwc_to_nchw(hip.view(plan.g_in), st.dtype, gx.data_ptr(), B, net.num_in_ch, H, W, hip.stream_ptr()),
                      "ssr_nhwc_to_nchw")
        if iog:
            gosm = torch.empty(Bo, 3, oplan.H, oplan.W, device=gy.device)
            hip.check(lib.ssr_nhwc_to_nchw(hip.view(oplan.g_in), hip.F32, gosm.data_ptr(), Bo, 3, oplan.H, oplan.W, hip.stream_ptr()),
                      "ssr_nhwc_to_nchw")
        return (None, gx, gosm, *net.grads_from_arena(needs))


@ARCH_REGISTRY.register()
class OSMObjDiscriminator(HipNet):
    def __init__(self, num_in_ch, num_feat=64, skip_connection=True, compute_dtype="fp32"):
        if hip.dtype_code(compute_dtype) == hip.BF16:
            raise NotImplementedError("OSMObjDiscriminator: compute_dtype 'bf16' is not implemented (the object branch is fp32 storage only); "
                                      "use fp32, fp32x3, fp32f or fp32h")
        super().__init__(engine.discriminator_specs(num_in_ch, num_feat), compute_dtype, rdb_prefix="\0")
        self.num_in_ch, self.num_feat, self.skip_connection = num_in_ch, num_feat, skip_connection
        self._ospecs = engine.object_branch_specs()
        for s in self._ospecs:
            self.add_module(s.name, ConvParams(s, "default"))
        for name, c in engine.OBJ_ATTENTION:
            self.add_module(name, _AttentionParams(c))
        # the reference's registration order (:49-69): it is the order of state_dict() and of parameters()
        order = ["o_conv1", "o_conv2", "o_attention1", "o_conv3", "o_attention2", "o_conv4"] + [f"conv{i}" for i in range(10)]
        self._modules = OrderedDict((k, self._modules[k]) for k in order)
        self._ostore = None
        self._oplans = {}

    # ---- two arenas: the U-Net half in the network's mode, the object branch in fp32 ----
    def store(self) -> engine.ParamStore:
        p0, pu = self.o_conv1.weight, self.conv0.weight
        if not p0.is_cuda:
            raise hip.HipLibraryError("this network runs only on the GPU through libssr_hip.so (no CPU path): "
                                      "move it with .to('cuda') / .cuda()")
        st, ost = self._store, self._ostore
        if (st is not None and st.device == p0.device and p0.data_ptr() == ost.ptr("o_conv1.weight")
                and pu.data_ptr() == st.ptr("conv0.weight")):
            return st
        hip.lib()
        st = engine.ParamStore(self._specs, hip.dtype_code(self.compute_dtype), device=p0.device)
        ost = engine.ParamStore(self._ospecs, hip.F32, device=p0.device, extras=engine.object_branch_extras())
        with torch.no_grad():
            for key, p in self.named_parameters():
                arena = ost if key.startswith("o_") else st
                arena.tensor(key).copy_(p.data)
                p.data = arena.tensor(key)
            for s in self._specs:
                if s.sn:
                    leaf = self._leaf(s.name)
                    st.u[s.name].copy_(leaf.weight_u)
                    st.v[s.name].copy_(leaf.weight_v)
                    leaf.weight_u = st.u[s.name]
                    leaf.weight_v = st.v[s.name]
        self._store, self._ostore = st, ost
        self._plans.clear()
        self._oplans.clear()
        self._packed_version = None
        return st

    def grads_from_arena(self, needs):
        st, ost = self._store, self._ostore
        out = []
        for k, need in zip(self.param_keys(), needs):
            arena = ost if k.startswith("o_") else st
            out.append(arena.tensor(k, arena.grad).clone() if need else None)
        return out

    def plan(self, B, H, W):
        key = (B, H, W)
        if key not in self._plans:
            p = engine.DiscriminatorPlan(self._store, B, H, W, num_in_ch=self.num_in_ch, num_feat=self.num_feat,
                                         skip_connection=self.skip_connection)
            xin = torch.zeros(B, H, W, p.cdp, dtype=hip.torch_dtype(self._store.dtype), device=self._store.device)
            self._plans[key] = (p, xin)
        return self._plans[key]

    def object_plan(self, Bo, H, W):
        key = (Bo, H, W)
        if key not in self._oplans:
            self._oplans[key] = engine.ObjectBranchPlan(self._ostore, Bo, H, W)
        return self._oplans[key]

    def forward(self, x, osm_objs):
        if osm_objs.dim() != 4 or osm_objs.shape[1] != 3 or osm_objs.shape[2] not in engine.OBJ_SIZES or osm_objs.shape[3] not in engine.OBJ_SIZES:
            raise ValueError(f"OSMObjDiscriminator: osm_objs of shape {tuple(osm_objs.shape)}; supported are [Bo, 3, H, W] with "
                             f"H, W in {engine.OBJ_SIZES} (the reference's model feeds 32 x 32 crops)")
        return _OSMDiscriminatorFn.apply(self, x, osm_objs, *self.parameters())
