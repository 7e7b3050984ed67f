"""OSMObjESRGANModel on MI355X - SSRESRGANModel plus the object-aware discriminator terms of the reference's
ssr/models/osm_objs_esrgan_model.py: same registry name, same option keys.

    osm_obj_weight                       weight of the three object GAN terms (:45)
    datasets.train.osm_objs_path         osm_chips_to_masks.json: {chip: {class: [[x1, y1, x2, y2], ...]}}, loaded once (:41-42)
    datasets.train.n_osm_objs            objects sampled per image and step (:46)
    network_d.type: OSMObjDiscriminator  required
    osm_obj_resize_antialias             ours (default false): torchvision's resize with or without antialiasing

feed_data takes `Chip` / `Phase` besides the images: a training batch looks its chips' boxes up, repairs and slice-resolves them
(osm_reference.resolve_boxes), draws n_osm_objs per image from Python's global `random` exactly as the reference does
(osm_reference.sample_objects) and hands the chosen boxes to the step (osm_train_step.OSMObjTrainStep.set_boxes); batches of other
phases carry none.  An empty crop - on which the reference crashes inside resize - raises ValueError naming the chip, on the host,
before anything is uploaded.  Validation, test(), checkpoints (net_d: the reference's 50 keys; optimizer_d follows that parameter
order) and schedulers are SSRESRGANModel's.

Refused by name (NotImplementedError): train.clip_opt / train.ldl_opt (as SSRESRGANModel), compute_dtype bf16, world size > 1, a training
batch of another shape than the first."""
from __future__ import annotations

import json
import os
import random
from dataclasses import dataclass

from .. import hip, osm_reference
from ..registry import MODEL_REGISTRY
from ..train_step import StepConfig
from .ssr_esrgan_model import SSRESRGANModel, train_config_from_opt


@dataclass
class OSMObjConfig:
    step: StepConfig
    osm_obj_weight: float
    n_osm_objs: int
    osm_objs_path: str
    antialias: bool


def osm_config_from_opt(opt: dict) -> OSMObjConfig:
    """Everything OSMObjESRGANModel reads from an option file beyond SSRESRGANModel, validated without a GPU.  The step's own
    settings go through train_config_from_opt, refusals included (train.clip_opt and train.ldl_opt raise there, by name)."""
    net_d = opt.get("network_d") or {}
    if net_d.get("type") != "OSMObjDiscriminator":
        raise NotImplementedError(f"network_d.type={net_d.get('type')!r}: OSMObjESRGANModel needs OSMObjDiscriminator (its forward takes the object crops)")
    dtype = (opt.get("network_g") or {}).get("compute_dtype", opt.get("compute_dtype", "fp32h"))
    if hip.dtype_code(dtype) == hip.BF16:
        raise NotImplementedError("OSMObjESRGANModel: compute_dtype 'bf16' is not implemented (OSMObjDiscriminator's object branch is fp32 "
                                  "storage only); use fp32, fp32x3, fp32f or fp32h")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if opt.get("dist", False):
        world = int(opt.get("world_size", world))
    if world > 1:
        raise NotImplementedError(f"OSMObjESRGANModel: world size {world} is not implemented (data-parallel training of this model); "
                                  "run it on one GPU")
    if (opt.get("train") or {}).get("clip_opt"):
        raise NotImplementedError("train.clip_opt: OSMObjESRGANModel does not run the CLIP loss (SSRESRGANModel does)")
    train_ds = (opt.get("datasets") or {}).get("train") or {}
    for k in ("osm_objs_path", "n_osm_objs"):
        if train_ds.get(k) is None:
            raise KeyError(f"datasets.train.{k}: OSMObjESRGANModel reads it (osm_objs_esrgan_model.py:41-46)")
    if "osm_obj_weight" not in opt:
        raise KeyError("osm_obj_weight: OSMObjESRGANModel reads it (osm_objs_esrgan_model.py:45)")
    n = int(train_ds["n_osm_objs"])
    if n < 1:
        raise ValueError(f"datasets.train.n_osm_objs={n}: at least one object per image")
    return OSMObjConfig(step=train_config_from_opt(opt), osm_obj_weight=float(opt["osm_obj_weight"]), n_osm_objs=n,
                        osm_objs_path=train_ds["osm_objs_path"], antialias=bool(opt.get("osm_obj_resize_antialias", False)))


@MODEL_REGISTRY.register()
class OSMObjESRGANModel(SSRESRGANModel):
    D_ARCH = "OSMObjDiscriminator"

    def __init__(self, opt: dict):
        self.osm = osm_config_from_opt(opt) if opt.get("is_train", True) else None      # option errors surface before the GPU is needed
        super().__init__(opt)
        self.osm_obj_data = None
        if self.is_train:
            with open(self.osm.osm_objs_path) as f:
                self.osm_obj_data = json.load(f)
        self._have_boxes = False

    def _build_step(self, B, h, w):
        from ..osm_train_step import OSMObjTrainStep
        return OSMObjTrainStep(self.g_kwargs, self.d_kwargs, B, h, w, self.compute_dtype, self.cfg, n_osm_objs=self.osm.n_osm_objs,
                               osm_obj_weight=self.osm.osm_obj_weight, antialias=self.osm.antialias, dp=self.dp)

    def _new_net_d(self):
        from ..archs.osm_obj_discriminator_arch import OSMObjDiscriminator
        return OSMObjDiscriminator(**self.d_kwargs)

    @staticmethod
    def _net_d_state_dict(ts):
        return ts.d_state_dict()

    @staticmethod
    def _optimizer_slots(o):
        if not hasattr(o, "parts"):
            return SSRESRGANModel._optimizer_slots(o)
        from ..osm_train_step import object_keys
        main, obj = o.parts         # net_d.named_parameters(): the object branch first, then the U-Net half
        return [(obj.store, k, obj) for k in object_keys(obj.store)] + [(main.store, k, main) for k in main.store.offsets]

    def _ensure(self, B, h, w):
        if self.ts is not None and (self.ts.B, self.ts.h, self.ts.w) != (B, h, w):
            raise NotImplementedError(f"OSMObjESRGANModel: a training batch of shape {(B, h, w)} after {(self.ts.B, self.ts.h, self.ts.w)}: "
                                      "the step is built for one batch shape (the training loader drops a ragged last batch)")
        super()._ensure(B, h, w)

    def feed_data(self, data: dict):
        super().feed_data(data)
        if not self.is_train or self._validating:
            return
        phase = data.get("Phase", "train")
        phase = phase if isinstance(phase, str) else phase[0]
        self._have_boxes = False
        if phase != "train":             # (:135-138: chip_objs only for training batches)
            return
        H, W, n = self.ts.H, self.ts.W, self.osm.n_osm_objs
        chips = [data["Chip"]] if isinstance(data["Chip"], str) else list(data["Chip"])
        boxes, self.chosen = [], []
        for b, chip in enumerate(chips):
            chip_objs = self.osm_obj_data[chip]
            resolved = osm_reference.resolve_boxes(osm_reference.flatten_objects(chip_objs), H, W, chip)     # every box: the reference resizes all
            idx = osm_reference.sample_objects(chip_objs, n, random)
            self.chosen.append(idx)
            boxes += [(b,) + resolved[i] for i in idx]
        self.ts.set_boxes(boxes)
        self._have_boxes = True

    def optimize_parameters(self, current_iter: int):
        if not self._have_boxes:
            raise RuntimeError("OSMObjESRGANModel.optimize_parameters: the last batch carried no objects (Phase != 'train')")
        super().optimize_parameters(current_iter)
