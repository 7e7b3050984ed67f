"""The train step of OSMObjESRGANModel: ESRGANTrainStep plus the object terms of the reference's
ssr/models/osm_objs_esrgan_model.py:163-200 (crops), :241-251 (generator term) and :285-308 (discriminator terms).

Per step, B * n_osm_objs OpenStreetMap boxes are cut out of the generated and of the real image, resized to 32 x 32
(csrc/obj_crop.hip) and judged by the object branch of OSMObjDiscriminator (engine.ObjectBranchPlan, exact fp32):

    G phase   crops of fake_in -> object branch -> l_g_gan_objs = osm_obj_weight * cri_gan(o_out, True, is_disc=False)
              -> object branch backward (input gradient only) -> the resize transpose ADDS that gradient into d_plan.g_in at every box,
              after the U-Net's backward wrote it and before the generator's backward reads it
    D phase   crops of real_in (the GAN target: it follows gan_gt_usm) and of fake_in -> l_d_real_objs, l_d_fake_objs; parameter
              gradients of the object branch go to its own arena

The boxes are data: they live in one device array that the crop kernels read when they run, filled from pinned host memory by
set_boxes() before each replay, outside the graph.  Bo = B * n_osm_objs is static, so the step stays one captured graph.

The discriminator has two arenas - the U-Net half in the step's arithmetic mode (d_store, as in the parent), the object branch in
fp32 (o_store) - and one optimiser over both (PairedOptimizer).  Only _phase_g / _phase_d / the optimiser phase and the loss slots are
overridden; the parent's launch lists, graphs and refusals are untouched."""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional, Sequence

import torch

from . import engine, hip
from .dp import DPContext
from .hip import view
from .train_step import ESRGANTrainStep, StepConfig, make_optimizer

# the reference's state_dict order of the object half (osm_obj_discriminator_arch.py:49-54); the U-Net half follows it
OBJ_MODULES = ("o_conv1", "o_conv2", "o_attention1", "o_conv3", "o_attention2", "o_conv4")
OBJ_LOSS_KEYS = ("l_g_gan_objs", "l_d_real_objs", "l_d_fake_objs")


def object_keys(o_store: engine.ParamStore):
    """the object branch's keys in the reference's state_dict order (the arena itself holds the attention blocks behind the convolutions)"""
    return [k for m in OBJ_MODULES for k in o_store.offsets if k.startswith(m + ".")]


class PairedOptimizer:
    """One optimiser over the discriminator's two arenas.  The update rules run per element, so two launches are the arithmetic of
    one.  The non-finite guard makes ONE decision: before either update both gradient arenas are scanned into BOTH flags (a flag is
    only ever set by a scan), so either both halves step or neither does; `skipped` is the U-Net half's counter - such a step counts
    once."""

    def __init__(self, main, obj):
        self.main, self.obj = main, obj
        self.parts = (main, obj)
        self.spec, self.guard, self.ema = main.spec, main.guard, None
        self.step, self.skipped = main.step, main.skipped
        self._srcs = (C.c_void_p * 2)(main.store.grad.data_ptr(), obj.store.grad.data_ptr())
        self._ns = (C.c_int64 * 2)(main.store.numel, obj.store.numel)

    def set_lr(self, lr: float):
        self.main.set_lr(lr)
        self.obj.set_lr(lr)

    def update(self, grad_scale: float = 1.0):
        if self.guard:
            for o in self.parts:
                hip.check(hip.lib().ssr_nonfinite_scan(self._srcs, self._ns, 2, o.flag.data_ptr(), hip.stream_ptr()), "ssr_nonfinite_scan")
        self.main.update(grad_scale)
        self.obj.update(grad_scale)


class OSMObjTrainStep(ESRGANTrainStep):
    def __init__(self, g_kwargs: Dict, d_kwargs: Dict, B: int, h: int, w: int, dtype="fp32", cfg: StepConfig = StepConfig(),
                 n_osm_objs: int = 1, osm_obj_weight: float = 1.0, antialias: bool = False, dp: Optional[DPContext] = None,
                 use_graph: bool = True, **kw):
        if hip.dtype_code(dtype) == hip.BF16:
            raise NotImplementedError("OSMObjTrainStep: compute_dtype 'bf16' is not implemented (the object branch and its crops are fp32 "
                                      "storage only); use fp32, fp32x3, fp32f or fp32h")
        if dp is not None and dp.active:
            raise NotImplementedError(f"OSMObjTrainStep: world size {dp.world} is not implemented (data-parallel training of the "
                                      "OSM-object model: the object branch's gradients are not exchanged); run on one GPU")
        if int(n_osm_objs) < 1:
            raise ValueError(f"n_osm_objs={n_osm_objs}: at least one object per image")
        super().__init__(g_kwargs, d_kwargs, B, h, w, dtype, cfg, dp=None, use_graph=use_graph, **kw)
        self.n_osm_objs, self.osm_obj_weight, self.antialias = int(n_osm_objs), float(osm_obj_weight), bool(antialias)
        self.Bo = B * self.n_osm_objs
        dev = self.g_store.device
        with engine.deterministic_mode(self.det):
            self.o_store = engine.ParamStore(engine.object_branch_specs(), hip.F32, device=dev, extras=engine.object_branch_extras())
            self.o_plan = engine.ObjectBranchPlan(self.o_store, self.Bo, hip.OBJ_CROP, hip.OBJ_CROP)
            main = self.opt_d
            obj = make_optimizer(self.o_store, cfg.optim_d, cfg.lr_d, cfg.betas_d or cfg.betas, cfg.eps, 0.0, self.nonfinite_guard)
            self.opt_d = PairedOptimizer(main, obj)
        self.obj_losses = torch.zeros(len(OBJ_LOSS_KEYS) * self.loss_stride, dtype=torch.float32, device=dev)
        # boxes (b, x1, y1, x2, y2) of the Bo objects, then first[B + 1] (objects are grouped by image: n_osm_objs each)
        n = 5 * self.Bo + B + 1
        self._boxes_host = torch.zeros(n, dtype=torch.int32).pin_memory()
        self._boxes_dev = torch.zeros(n, dtype=torch.int32, device=dev)
        self._boxes_host[5 * self.Bo:] = torch.arange(B + 1, dtype=torch.int32) * self.n_osm_objs
        self._boxes_set = False
        self._boxes_copied = torch.cuda.Event()

    # ------------------------------------------------------------------ state
    def load_state(self, g_sd, d_sd, reset_ema: bool = True):
        super().load_state(g_sd, d_sd, reset_ema)
        self.o_store.load_state_dict(d_sd)

    def d_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """net_d's checkpoint: the reference's 50 keys in its order"""
        out = OrderedDict((k, self.o_store.tensor(k).clone()) for k in object_keys(self.o_store))
        out.update(self.d_store.state_dict())
        return out

    def d_param_slots(self):
        """(store, key) of net_d's parameters in named_parameters() order: what optimizer_d's state follows"""
        return [(self.o_store, k) for k in object_keys(self.o_store)] + [(self.d_store, k) for k in self.d_store.offsets]

    # ------------------------------------------------------------------ data
    def set_boxes(self, boxes: Sequence[Sequence[int]]):
        """boxes: Bo rows (b, x1, y1, x2, y2), n_osm_objs per image in batch order, already fixed up and slice-resolved
        (osm_reference.resolve_boxes).  Checked here, on the host, before anything is uploaded; one asynchronous copy from pinned
        memory, in stream order before the next replay."""
        t = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 5)
        if t.shape[0] != self.Bo:
            raise ValueError(f"{t.shape[0]} boxes for B * n_osm_objs = {self.Bo}")
        for o, (b, x1, y1, x2, y2) in enumerate(t.tolist()):
            if b != o // self.n_osm_objs or not (0 <= x1 < x2 <= self.W and 0 <= y1 < y2 <= self.H):
                raise ValueError(f"object {o}: box {(b, x1, y1, x2, y2)} is not a crop of image {o // self.n_osm_objs} of {self.H} x {self.W}")
            if max(x2 - x1, y2 - y1) > hip.OBJ_MAX_SIDE:
                raise ValueError(f"object {o}: box {(b, x1, y1, x2, y2)} has a side above {hip.OBJ_MAX_SIDE} (SSR_OBJ_MAX_SIDE)")
        if self._boxes_set:
            self._boxes_copied.synchronize()            # the previous upload has read the pinned buffer (it was queued a whole step ago)
        self._boxes_host[:5 * self.Bo] = t.flatten()
        self._boxes_dev.copy_(self._boxes_host, non_blocking=True)
        self._boxes_copied.record()
        self._boxes_set = True

    def step(self, current_iter: Optional[int] = None):
        if not self._boxes_set:
            raise RuntimeError("OSMObjTrainStep.step() before set_boxes(): the step has no objects to cut out")
        super().step(current_iter)

    # ------------------------------------------------------------------ phases
    def _crop(self, img: torch.Tensor):
        bp = self._boxes_dev.data_ptr()
        hip.check(hip.lib().ssr_obj_crop_resize_fwd(view(img), self.dt, self.B, self.H, self.W, bp, self.Bo, view(self.o_plan.xin),
                                                    int(self.antialias), hip.stream_ptr()), "ssr_obj_crop_resize_fwd")

    def _obj_gan(self, target_is_real: bool, weight: float, slot: int, is_disc: bool):
        """cri_gan on o_out [Bo, 1, 2, 2]: the two squeeze(-1) of the reference are no-ops at 2 x 2, the mean is over Bo * 4 logits"""
        cfg, p = self.cfg, self.o_plan
        n = self.Bo * p.hs[4][0] * p.hs[4][1]
        target = cfg.real_label if target_is_real else cfg.fake_label
        loss_ptr = self.obj_losses.data_ptr() + 4 * self.loss_stride * slot
        if cfg.gan_type == "vanilla":
            hip.check(hip.lib().ssr_bce_logits_loss(view(p.out), view(p.d_out), self.loss_dt, n, target, weight, loss_ptr, None,
                                                    hip.stream_ptr()), "ssr_bce_logits_loss (objects)")
        else:
            hip.check(hip.lib().ssr_gan_loss(view(p.out), view(p.d_out), self.loss_dt, n, hip.GAN_TYPES[cfg.gan_type], int(target_is_real),
                                             int(is_disc), target, weight, loss_ptr, None, hip.stream_ptr()), "ssr_gan_loss (objects)")

    def _phase_g(self, run_bwd: bool = True):
        cfg = self.cfg
        self._zero(self.obj_losses)
        super()._phase_g(run_bwd=False)                 # ... up to the U-Net's backward into d_plan.g_in (:245, D frozen)
        self.o_store.pack()
        self._crop(self.fake_in)                        # gen_objs (:179-181, :198)
        self.o_plan.fwd.run()                           # obj_pred (:241)
        self._obj_gan(True, self.osm_obj_weight * cfg.gan_weight, 0, is_disc=False)     # l_g_gan_objs (:247)
        self.o_plan.backward_plan(param_grads=False, input_grad=True).run()
        hip.check(hip.lib().ssr_obj_crop_resize_bwd(view(self.o_plan.g_in), self._boxes_dev.data_ptr(),
                                                    self._boxes_dev.data_ptr() + 4 * 5 * self.Bo, self.Bo, view(self.d_plan.g_in), self.dt,
                                                    self.B, self.H, self.W, 1.0, int(self.antialias), hip.stream_ptr()),
                  "ssr_obj_crop_resize_bwd")
        if run_bwd:
            self.g_plan.bwd.run()

    def _phase_g_skipped(self):
        self._zero(self.obj_losses)
        super()._phase_g_skipped()

    def _phase_d(self):
        w = self.osm_obj_weight
        self._zero(self.o_store.grad)
        self.o_store.pack()
        self._crop(self.real_in)                        # gt_objs: crops of gan_gt (:178, :285)
        self.o_plan.fwd.run()
        self._obj_gan(True, w, 1, is_disc=True)         # l_d_real_objs (:288)
        self.o_plan.backward_plan(param_grads=True, input_grad=False).run()
        self._crop(self.fake_in)                        # gen_objs.detach() (:298)
        self.o_plan.fwd.run()
        # l_d_fake_objs: the target is True in the reference's text (:301: cri_gan(fake_obj_pred_avg, True, is_disc=True)), not False
        # as for the whole image two lines below it; reproduced as written
        self._obj_gan(True, w, 2, is_disc=True)
        self.o_plan.backward_plan(param_grads=True, input_grad=False).run()
        super()._phase_d()

    # ------------------------------------------------------------------ results
    def log(self) -> "OrderedDict[str, float]":
        """the reference's keys in the order its loss_dict gets them (:208-306).  `l_d_real += l_d_real_objs` (:294) and
        `l_d_fake += l_d_fake_objs` (:307) are in-place adds on the tensors loss_dict already holds: the logged l_d_real / l_d_fake
        are the sums."""
        base = super().log()
        n = len(OBJ_LOSS_KEYS)
        o = (self.obj_losses if not self.det else self.obj_losses.view(n, self.loss_stride).double().sum(1)).tolist()
        out = OrderedDict()
        for k in ("l_g_pix", "l_g_percep", "l_g_style", "l_g_ssim", "l_g_gan"):
            if k in base:
                out[k] = base[k]
        out["l_g_gan_objs"] = o[0]
        out["l_d_real"], out["l_d_real_objs"], out["out_d_real"] = base["l_d_real"] + o[1], o[1], base["out_d_real"]
        out["l_d_fake"], out["l_d_fake_objs"], out["out_d_fake"] = base["l_d_fake"] + o[2], o[2], base["out_d_fake"]
        return out

    def object_crops(self, which: str = "fake") -> torch.Tensor:
        """[Bo, 3, 32, 32]: the current boxes cut out of the generated ("fake") or the real ("real": the GAN target) image as the buffers
        hold them now - one eager crop launch into the object plan's input, for inspection between steps"""
        self._crop(self.fake_in if which == "fake" else self.real_in)
        return self.o_plan.xin[..., :3].permute(0, 3, 1, 2).contiguous()
