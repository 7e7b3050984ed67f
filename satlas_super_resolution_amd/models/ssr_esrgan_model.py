"""SSRESRGANModel on MI355X — the model plugin the training loop drives
(/root/reference/ssr/train.py:62-65,106-133), mirroring /root/reference/ssr/models/ssr_esrgan_model.py:

    feed_data(:104-117)  optimize_parameters(:119-233)  test(:235-244)  get_current_visuals(:246-252)
    nondist_validation(:269-352)
    + the BasicSR BaseModel methods train.py calls: update_learning_rate, get_current_learning_rate,
      get_current_log, save, resume_training, validation.

Same registry name and the same `opt` dictionary (YAML) keys.  Instead of autograd over ~41k ATen ops per
step, optimize_parameters() replays the fused HIP-graph step of train_step.ESRGANTrainStep.
Scope: BasicSR's pixel (L1 / MSE / Charbonnier) and GAN (vanilla / lsgan / wgan / wgan_softplus / hinge) losses (+ VGG19 perceptual: feature and Gram-style terms; + SSIM; + the CLIP loss on ViT-B-16-SigLIP-256) losses, USM-sharpened ground truth,
`feed_disc_lr` and `old_hr` discriminator inputs, BasicSR's optimizers (Adam / AdamW / SGD / RMSprop with their options) and
schedulers (MultiStepRestartLR, CosineAnnealingRestartLR; optimizers.py).  Anything this path does not implement raises
NotImplementedError naming the option (the ldl loss, other CLIP-loss towers, Adamax / ASGD / Rprop, other schedulers) — nothing is silently ignored."""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch

from .. import hip, optimizers
from ..dp import init_distributed
from ..registry import MODEL_REGISTRY
from ..train_step import ESRGANTrainStep, StepConfig


def _arch_kwargs(net_opt: dict, expect: str) -> dict:
    kw = {k: v for k, v in net_opt.items() if k != "type"}
    if net_opt.get("type", expect) != expect:
        raise NotImplementedError(f"network type {net_opt.get('type')!r}: only {expect} is on the MI355X hot path")
    return kw


def step_config_from_opt(opt: dict) -> StepConfig:
    """The knobs init_training_settings reads (ssr_esrgan_model.py:33-102; esrgan_s2naip_urban.yml:96-147), validated:
    an option this path cannot honour raises instead of being dropped."""
    train_opt = opt.get("train", {})
    for k in ("ldl_opt", "ssim_opt", "clip_opt"):
        if train_opt.get(k):
            raise NotImplementedError(f"train.{k}: outside the MI355X hot path (SURVEY.md §8f)")
    pix, gan = train_opt.get("pixel_opt"), train_opt.get("gan_opt") or {}
    if pix and pix.get("type", "L1Loss") != "L1Loss":
        raise NotImplementedError(f"train.pixel_opt.type={pix.get('type')!r}: only L1Loss")
    if pix and pix.get("reduction", "mean") != "mean":
        raise NotImplementedError("train.pixel_opt.reduction: only 'mean'")
    if gan.get("type", "GANLoss") != "GANLoss" or gan.get("gan_type", "vanilla") != "vanilla":
        raise NotImplementedError("train.gan_opt: only GANLoss with gan_type: vanilla")
    og, od = dict(train_opt.get("optim_g", {})), dict(train_opt.get("optim_d", {}))
    for name, o in (("optim_g", og), ("optim_d", od)):
        if o.get("type", "Adam") != "Adam":
            raise NotImplementedError(f"train.{name}.type={o.get('type')!r}: only Adam")
        if float(o.get("weight_decay", 0)) != 0.0:
            raise NotImplementedError(f"train.{name}.weight_decay != 0")
        if o.get("amsgrad", False):
            raise NotImplementedError(f"train.{name}.amsgrad")
    sch = train_opt.get("scheduler", {})
    if sch and sch.get("type", "MultiStepLR") not in ("MultiStepLR", "MultiStepRestartLR"):
        raise NotImplementedError(f"train.scheduler.type={sch.get('type')!r}: only MultiStepLR / MultiStepRestartLR")
    if sch and (list(sch.get("restarts", [0])) != [0] or list(sch.get("restart_weights", [1])) != [1]):
        raise NotImplementedError("train.scheduler restarts")
    perc = train_opt.get("perceptual_opt")
    return StepConfig(
        l1_weight=float(pix.get("loss_weight", 1.0)) if pix else 0.0,    # no pixel_opt: cri_pix = None (:47-50)
        gan_weight=float(gan.get("loss_weight", 0.1)),
        lr_g=float(og.get("lr", 1e-4)), lr_d=float(od.get("lr", 1e-4)),
        betas=tuple(og.get("betas", (0.9, 0.999))), betas_d=tuple(od.get("betas", (0.9, 0.999))),
        eps=float(og.get("eps", 1e-8)), ema_decay=float(train_opt.get("ema_decay", 0)),
        net_d_iters=int(train_opt.get("net_d_iters", 1)), net_d_init_iters=int(train_opt.get("net_d_init_iters", 0)),
        feed_disc_lr=bool(opt.get("feed_disc_lr", False)),
        # `if self.opt['l1_gt_usm'] is False: l1_gt = self.gt` (ssr_esrgan_model.py:121-129): sharpened unless exactly False
        l1_gt_usm=opt.get("l1_gt_usm", False) is not False, gan_gt_usm=opt.get("gan_gt_usm", False) is not False,
        percep_gt_usm=opt.get("percep_gt_usm", False) is not False,
        real_label=float(gan.get("real_label_val", 1.0)), fake_label=float(gan.get("fake_label_val", 0.0)),
        perceptual=dict(perc) if perc else None,
        deterministic=bool(opt.get("deterministic", False)))   # ours: fixed-order reductions only (bit-identical runs; train_step.StepConfig)


def train_config_from_opt(opt: dict) -> StepConfig:
    """step_config_from_opt plus `train.ssim_opt` (SSIMLoss: ssr/losses/basic_loss.py:50-60, built at ssr_esrgan_model.py:62-65),
    `train.clip_opt` (CLIPLoss: clip_loss.check_clip_opt validates the block and finds the tower's weights; StepConfig.clip) and
    BasicSR's other pixel and GAN losses (`pixel_opt.type`: MSELoss, CharbonnierLoss; `gan_opt.gan_type`: lsgan, wgan, wgan_softplus,
    hinge - basicsr/losses/basic_loss.py, gan_loss.py): what SSRESRGANModel configures its step from.

    Why two functions: step_config_from_opt's refusals of `ssim_opt`, of `wgan` and of `MSELoss` are pinned by
    tests/test_host_boundary.py, so it stays as it is; this one validates those settings, hands step_config_from_opt a copy of `opt`
    without the block / with the two types set back to L1Loss and vanilla, and sets StepConfig.ssim / .pixel_type / .pixel_eps /
    .gan_type on the result.  Folding the two into one goes with a change of that test.

    ssim_opt holds `type: SSIMLoss` and optionally `loss_weight` (default 1.0, as SSIMLoss.__init__); the window (5 x 5) is fixed in
    the reference's forward.  pixel_opt holds `type`, `loss_weight`, `reduction: mean` and, for CharbonnierLoss, `eps` (default 1e-12) -
    the constructors' arguments.  Any other type or key raises NotImplementedError naming it.

    The same pattern for `optim_g` / `optim_d` (BasicSR get_optimizer: Adam, AdamW, SGD, RMSprop with the numeric and boolean arguments
    of the torch.optim constructors - optimizers.normalize_optim) and for `scheduler` (restarts / restart_weights of MultiStepRestartLR,
    CosineAnnealingRestartLR - optimizers.Schedule, which SSRESRGANModel evaluates): step_config_from_opt sees plain Adam blocks
    and no scheduler where it would refuse; StepConfig.optim_g / .optim_d carry the full description unless the block IS plain Adam
    (weight_decay 0, no amsgrad), which stays on the launches it always had."""
    train_opt = opt.get("train", {}) or {}
    rest_train = dict(train_opt)
    ssim = None
    so = train_opt.get("ssim_opt")
    if so:
        if so.get("type") != "SSIMLoss":
            raise NotImplementedError(f"train.ssim_opt.type={so.get('type')!r}: only SSIMLoss")
        for k in so:
            if k not in ("type", "loss_weight"):
                raise NotImplementedError(f"train.ssim_opt.{k}: SSIMLoss takes loss_weight only")
        del rest_train["ssim_opt"]
        ssim = {"loss_weight": float(so.get("loss_weight", 1.0))}
    clip = None
    co = train_opt.get("clip_opt")
    if co:      # CLIPLoss (ssr/losses/basic_loss.py:19-48, built at ssr_esrgan_model.py:77-80): clip_loss.check_clip_opt names every refusal
        from ..clip_loss import check_clip_opt
        clip = check_clip_opt(co)
        dtype = (opt.get("network_g") or {}).get("compute_dtype", opt.get("compute_dtype", "fp32h"))
        if hip.dtype_code(dtype) == hip.BF16:
            raise NotImplementedError("train.clip_opt with compute_dtype 'bf16': the tower reads fp32 images; use fp32, fp32x3, fp32f or fp32h")
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if opt.get("dist", False):
            world = int(opt.get("world_size", world))
        if world > 1:
            raise NotImplementedError(f"train.clip_opt with world size {world}: l_clip_sim is not part of the cross-rank reduction of the "
                                      "logged scalars; run it on one GPU")
        del rest_train["clip_opt"]
    pixel_type, pixel_eps = "L1Loss", 1e-12
    pix = train_opt.get("pixel_opt")
    if pix:
        pixel_type = pix.get("type", "L1Loss")
        if pixel_type not in ("L1Loss",) + tuple(hip.PIXEL_KINDS):
            raise NotImplementedError(f"train.pixel_opt.type={pixel_type!r}: only L1Loss, MSELoss, CharbonnierLoss")
        takes = ("type", "loss_weight", "reduction") + (("eps",) if pixel_type == "CharbonnierLoss" else ())
        for k in pix:
            if k not in takes:
                raise NotImplementedError(f"train.pixel_opt.{k}: {pixel_type} takes {', '.join(takes[1:])}")
        if pix.get("reduction", "mean") != "mean":
            raise NotImplementedError(f"train.pixel_opt.reduction={pix.get('reduction')!r}: only 'mean'")
        pixel_eps = float(pix.get("eps", 1e-12))
        if not pixel_eps >= 0.0:
            raise NotImplementedError(f"train.pixel_opt.eps={pix.get('eps')!r}: must be >= 0")
        rest_train["pixel_opt"] = {k: ("L1Loss" if k == "type" else v) for k, v in pix.items() if k != "eps"}
    gan_type = "vanilla"
    gan = train_opt.get("gan_opt")
    if gan:
        gan_type = gan.get("gan_type", "vanilla")
        if gan_type not in ("vanilla",) + tuple(hip.GAN_TYPES):
            raise NotImplementedError(f"train.gan_opt.gan_type={gan_type!r}: only vanilla, lsgan, wgan, wgan_softplus, hinge")
        rest_train["gan_opt"] = dict(gan, gan_type="vanilla")
    specs = {}
    for name in ("optim_g", "optim_d"):
        spec = optimizers.normalize_optim(name, train_opt.get(name))
        if optimizers.is_plain_adam(spec) and not spec.get("decoupled_weight_decay"):
            specs[name] = None          # step_config_from_opt reads the block itself, as ever
            continue
        specs[name] = spec
        rest_train[name] = {"type": "Adam", "lr": spec["lr"], "betas": spec.get("betas", (0.9, 0.999)), "eps": spec.get("eps", 1e-8)}
    sched = optimizers.Schedule(train_opt.get("scheduler"), train_opt.get("total_iter"))     # validates; the model builds its own
    if not sched.plain_multistep:
        rest_train.pop("scheduler", None)
    rest = dict(opt)
    rest["train"] = rest_train
    cfg = step_config_from_opt(rest)
    cfg.ssim, cfg.pixel_type, cfg.pixel_eps, cfg.gan_type = ssim, pixel_type, pixel_eps, gan_type
    cfg.optim_g, cfg.optim_d = specs["optim_g"], specs["optim_d"]
    cfg.clip = clip
    return cfg


@MODEL_REGISTRY.register()
class SSRESRGANModel:
    D_ARCH = "SSR_UNetDiscriminatorSN"      # network_d.type this model drives (a subclass with another discriminator names its own)

    def __init__(self, opt: dict):
        self.opt = opt
        self.is_train = opt.get("is_train", True)
        if not torch.cuda.is_available():
            raise hip.HipLibraryError("SSRESRGANModel needs an MI355X (no CPU fallback)")
        hip.lib()
        self.device = torch.device("cuda")
        self.dp = init_distributed() if opt.get("dist", False) else None
        self.g_kwargs = _arch_kwargs(opt["network_g"], "SSR_RRDBNet")
        # default arithmetic: fp32h - fp16-split forward (22 bits per operand: outputs and LeakyReLU decisions of an fp32 evaluation),
        # split-bf16 backward: the fastest mode inside EVERY gate of the reference (outputs and parameter gradients at 1e-3, hip.F32H);
        # `compute_dtype: fp32f` has the forward in exact fp32 (no fp16 range: activations beyond 65504), `fp32` is exact throughout,
        # `fp32x3` (outputs inside the gate) / `bf16` are the modes outside the gradient gate
        self.compute_dtype = self.g_kwargs.pop("compute_dtype", opt.get("compute_dtype", "fp32h"))
        self.feed_disc_lr = bool(opt.get("feed_disc_lr", False))
        if self.is_train:      # test.py builds the model with is_train=False: generator only (SRGANModel.__init__ / init_training_settings)
            self.d_kwargs = _arch_kwargs(opt["network_d"], self.D_ARCH)
            self.d_kwargs.pop("compute_dtype", None)
            self.cfg = train_config_from_opt(opt)
        else:
            self.d_kwargs, self.cfg = None, StepConfig()
        train_opt = opt.get("train", {}) or {}
        self.schedule = optimizers.Schedule(train_opt.get("scheduler"), train_opt.get("total_iter") if self.is_train else None)
        self.ts = None
        self._pending_state = None         # resume_training() before the first batch built the step (train.py:64-65)
        self._infer = None                 # (store, plan) of test()
        self._validating = False
        self.log_dict = OrderedDict()
        self.lr = self.gt = self.output = None
        self.current_lrs = [self.cfg.lr_g, self.cfg.lr_d]
        self.metric_results = {}
        self.best_metric_results = {}

    # ---- plan creation is lazy: shapes come from the first batch ----
    def _ensure(self, B, h, w):
        if self.ts is not None and (self.ts.B, self.ts.h, self.ts.w) == (B, h, w):
            return
        old, self.ts, self._infer = self.ts, None, None
        carry = None
        if old is not None:     # a ragged last batch / another tile size: carry every piece of state over, then free the old step
            carry = dict(g=old.g_store.state_dict(), d=self._net_d_state_dict(old),
                         opt=[({k: t.clone() for k, t in o.arenas.items()}, o.step.clone(), o.skipped.clone()) for o in (old.opt_g, old.opt_d)],
                         ema=None if old.opt_g.ema is None else old.opt_g.ema.clone(), it=old.iter)
            del old
            import gc
            gc.collect()
            torch.cuda.empty_cache()
        self.ts = self._build_step(B, h, w)
        if carry is None:
            self._init_params()
        else:
            self.ts.load_state(carry["g"], carry["d"], reset_ema=False)
            for o, (arenas, s, k) in zip((self.ts.opt_g, self.ts.opt_d), carry["opt"]):
                for key, t in arenas.items():          # every state arena of the optimizer (exp_avg, ..., momentum_buffer, ...)
                    o.arenas[key].copy_(t)
                o.step.copy_(s); o.skipped.copy_(k)
            if carry["ema"] is not None:
                self.ts.opt_g.ema.copy_(carry["ema"])
            self.ts.iter = carry["it"]
        if self._pending_state is not None:
            self._apply_resume_state(self._pending_state)
            self._pending_state = None
        # the schedule lives on the host: a freshly built step starts at the base LR
        self.ts.opt_g.set_lr(self.current_lrs[0])
        self.ts.opt_d.set_lr(self.current_lrs[1])

    # ---- what a subclass with another discriminator replaces ----
    def _build_step(self, B, h, w):
        return ESRGANTrainStep(self.g_kwargs, self.d_kwargs, B, h, w, self.compute_dtype, self.cfg, dp=self.dp)

    def _new_net_d(self):
        from ..archs.discriminator_arch import SSR_UNetDiscriminatorSN
        return SSR_UNetDiscriminatorSN(**self.d_kwargs)

    @staticmethod
    def _net_d_state_dict(ts):
        return ts.d_store.state_dict()

    @staticmethod
    def _optimizer_slots(o):
        """(store, key, optimizer over that store) of the parameters an optimizer steps, in named_parameters() order"""
        return [(o.store, k, o) for k in o.store.offsets]

    def _init_params(self):
        from ..archs.rrdbnet_arch import SSR_RRDBNet
        path = self.opt.get("path", {})
        seed = self.opt.get("manual_seed")
        # initialise under a forked RNG: the caller's global stream (seeded manual_seed + rank by options.py:81 and consumed
        # by the dataloaders) is left untouched
        with torch.random.fork_rng(devices=[]):
            if seed is not None:
                torch.manual_seed(int(seed))
            g_sd = SSR_RRDBNet(**self.g_kwargs).state_dict()
            d_sd = self._new_net_d().state_dict()
        ema_sd = None
        if path.get("pretrain_network_g"):   # load_network(net_g, path, strict_load_g, param_key_g) + net_g_ema <- 'params_ema'
            ck = torch.load(path["pretrain_network_g"], map_location="cpu")
            g_sd = ck[path.get("param_key_g", "params")]
            ema_sd = ck.get("params_ema")     # init_training_settings: net_g_ema loads 'params_ema' (:39-49)
        if path.get("pretrain_network_d"):
            ck = torch.load(path["pretrain_network_d"], map_location="cpu")
            d_sd = ck[path.get("param_key_d", "params")]
        self.ts.load_state(g_sd, d_sd)
        if ema_sd is not None and self.ts.opt_g.ema is not None:
            for key in self.ts.g_store.offsets:
                self.ts.g_store.tensor(key, self.ts.opt_g.ema).copy_(ema_sd[key].to(self.device, torch.float32))
        if self.dp is not None:
            self.ts.sync_params_from_rank0(reset_ema=ema_sd is None)

    # ---- the methods train.py calls ----
    def feed_data(self, data: dict):
        """ssr_esrgan_model.py:104-117: uint8 tensors -> float/255 on the device."""
        lr = data["lr"].to(self.device, non_blocking=True).float()
        B, _, h, w = lr.shape
        if not self.is_train or (self._validating and self.ts is not None):
            # validation batches (usually of another size) only feed test(): the train step, its plans and graphs stay as they are
            self.lr = lr / 255
            self.gt = data["hr"].to(self.device, non_blocking=True).float() / 255 if "hr" in data else None
            return
        has_old = "old_hr" in data and "hr" in data
        if self.ts is None:
            self.cfg.old_hr = has_old      # the D input width is static: decided by the first training batch
        self._ensure(B, h, w)
        self.lr = lr / 255
        if "hr" in data:
            gt = data["hr"].to(self.device, non_blocking=True).float()
            self.gt = gt / 255
            old = data["old_hr"].to(self.device, non_blocking=True).float() if self.cfg.old_hr else None
            self.ts.feed_data(lr, gt, scale=1.0 / 255, old_hr=old)
        else:
            self.gt = None
            self.ts.g_plan.load_input(lr.contiguous(), 1.0 / 255)

    def optimize_parameters(self, current_iter: int):
        # the reference indexes these keys directly (KeyError when absent): ssr_esrgan_model.py:124-129
        _ = [self.opt["l1_gt_usm"], self.opt["percep_gt_usm"], self.opt["gan_gt_usm"]]   # applied in feed_data (StepConfig)
        self.ts.step(current_iter)
        self.output = None  # materialised lazily by get_current_visuals()

    def get_current_log(self):
        self.log_dict = self.ts.log()
        # the fp16-split forward of mode fp32h has fp16's range (include/ssr_hip.h, SSR_F32H): an activation beyond 65504 turns into NaN outputs.
        # The losses are read from the device here anyway: say what to do instead of logging NaN silently
        if self.compute_dtype == "fp32h" and any(isinstance(v, float) and not math.isfinite(v) for v in self.log_dict.values()):
            kept = (" Updates with non-finite gradients are skipped on the device: weights, Adam moments and step counts were left unchanged "
                    f"(skipped so far: {self.nonfinite_skips}).") if self.ts.nonfinite_guard else ""
            raise FloatingPointError("non-finite loss in compute_dtype fp32h: its forward convolutions run on fp16-split operands (|activation| < 65504, "
                                     "|weight| < 64); set `compute_dtype: fp32f` (exact fp32 forward, same gates) for this model." + kept)
        return self.log_dict

    @property
    def nonfinite_skips(self) -> dict:
        """updates skipped by the non-finite guard so far, per network (ESRGANTrainStep.nonfinite_skips; one device read)"""
        g, d = self.ts.nonfinite_skips() if self.ts is not None else (0, 0)
        return {"net_g": g, "net_d": d}

    def update_learning_rate(self, current_iter: int, warmup_iter: int = -1):
        """BasicSR BaseModel.update_learning_rate: the schedulers are stepped once per call from the second call on
        (last_epoch = current_iter - 1), MultiStepRestartLR multiplies by gamma when last_epoch reaches a milestone
        (esrgan_s2naip_urban.yml:109-112); during warm-up the LR is base * current_iter / warmup_iter.  The closed forms, restarts and
        CosineAnnealingRestartLR: optimizers.Schedule."""
        self.current_lrs = [self.schedule.lr(self.cfg.lr_g, current_iter, warmup_iter), self.schedule.lr(self.cfg.lr_d, current_iter, warmup_iter)]
        if self.ts is not None:
            self.ts.opt_g.set_lr(self.current_lrs[0])
            self.ts.opt_d.set_lr(self.current_lrs[1])

    def get_current_learning_rate(self):
        return [self.current_lrs[0]]

    def test(self):
        """:235-244 — forward with the EMA weights (net_g_ema) under no_grad."""
        from .. import engine
        ts = self.ts
        B, _, h, w = self.lr.shape
        key = (B, h, w)
        dt = ts.mode if ts is not None else hip.dtype_code(self.compute_dtype)      # the arithmetic MODE (fp32f: this forward is exact fp32)
        if self._infer is None or self._infer[0] != key:
            st = self._infer[1] if self._infer is not None else engine.ParamStore(engine.generator_specs(**self.g_kwargs), dt)
            if self._infer is None and ts is None:
                st.load_state_dict(self._test_weights())
            self._infer = (key, st, engine.GeneratorPlan(st, B, h, w, training=False, **self.g_kwargs))
        _, st, plan = self._infer
        if ts is not None:
            st.data.copy_(ts.opt_g.ema if ts.opt_g.ema is not None else ts.g_store.data)
        st.pack()
        plan.load_input(self.lr.contiguous(), 1.0)      # self.lr = lr/255 already (one rounding, as :107 of the reference)
        plan.fwd.run()
        self.output = plan.read_output()

    def _test_weights(self):
        """is_train=False (test.py): load_network(net_g, pretrain_network_g, strict_load_g, param_key_g); without a checkpoint the
        default initialisation under manual_seed, as constructing the reference model would give."""
        path = self.opt.get("path", {}) or {}
        if path.get("pretrain_network_g"):
            ck = torch.load(path["pretrain_network_g"], map_location="cpu")
            return ck[path.get("param_key_g", "params")]
        from ..archs.rrdbnet_arch import SSR_RRDBNet
        with torch.random.fork_rng(devices=[]):
            if self.opt.get("manual_seed") is not None:
                torch.manual_seed(int(self.opt["manual_seed"]))
            return SSR_RRDBNet(**self.g_kwargs).state_dict()

    def get_current_visuals(self):
        out = OrderedDict()
        out["lr"] = self.lr.detach().cpu()
        out["result"] = (self.output if self.output is not None else self.ts.output()).detach().cpu()
        if self.gt is not None:
            out["gt"] = self.gt.detach().cpu()
        return out

    # ---- checkpoints (BasicSR layout, loadable by either side) ----
    def _optimizer_state_dict(self, o, lr, betas):
        """torch.optim.Adam.state_dict() over the parameters in named_parameters() order (BasicSR setup_optimizers); the other
        optimizers (o.spec): optimizers.optimizer_state_dict."""
        slots = self._optimizer_slots(o)
        keys = [k for _, k, _ in slots]
        if o.spec is not None:
            per = [{a: st.tensor(k, t) for a, t in part.arenas.items()} for st, k, part in slots]
            return optimizers.optimizer_state_dict(o.spec, lr, per, int(o.step.item()))
        step = float(o.step.item())
        state = {i: {"step": torch.tensor(step), "exp_avg": st.tensor(k, part.exp_avg).detach().cpu().clone(),
                     "exp_avg_sq": st.tensor(k, part.exp_avg_sq).detach().cpu().clone()} for i, (st, k, part) in enumerate(slots)}
        group = {"lr": lr, "betas": tuple(betas), "eps": self.cfg.eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": lr,
                 "params": list(range(len(keys)))}
        return {"state": state, "param_groups": [group]}

    def _scheduler_state_dict(self, base_lr, lr, current_iter):
        """basicsr MultiStepRestartLR / CosineAnnealingRestartLR .state_dict() (= the scheduler's __dict__ minus the optimizer)."""
        return self.schedule.state_dict(base_lr, lr, current_iter)

    def save(self, epoch: int, current_iter: int):
        """BasicSR layout: net_g_{iter}.pth = {'params', 'params_ema'}, net_d_{iter}.pth = {'params'},
        training_states/{iter}.state = {'epoch', 'iter', 'optimizers': [Adam state_dicts], 'schedulers': [...]}."""
        if self.dp is not None and self.dp.rank != 0:
            return
        it = "latest" if current_iter == -1 else str(current_iter)
        path = self.opt.get("path", {})
        mdir, sdir = path.get("models", "experiments/models"), path.get("training_states", "experiments/training_states")
        os.makedirs(mdir, exist_ok=True)
        os.makedirs(sdir, exist_ok=True)
        cpu = lambda sd: OrderedDict((k, v.cpu()) for k, v in sd.items())
        g = {"params": cpu(self.ts.g_store.state_dict())}
        if self.ts.opt_g.ema is not None:
            g["params_ema"] = cpu(self.ts.ema_state_dict())
        torch.save(g, os.path.join(mdir, f"net_g_{it}.pth"))
        torch.save({"params": cpu(self._net_d_state_dict(self.ts))}, os.path.join(mdir, f"net_d_{it}.pth"))
        cfg = self.cfg
        state = {"epoch": epoch, "iter": current_iter,
                 "optimizers": [self._optimizer_state_dict(self.ts.opt_g, self.current_lrs[0], cfg.betas),
                                self._optimizer_state_dict(self.ts.opt_d, self.current_lrs[1], cfg.betas_d or cfg.betas)],
                 "schedulers": [self._scheduler_state_dict(cfg.lr_g, self.current_lrs[0], current_iter),
                                self._scheduler_state_dict(cfg.lr_d, self.current_lrs[1], current_iter)]}
        torch.save(state, os.path.join(sdir, f"{it}.state"))

    def resume_training(self, resume_state: dict):
        """BaseModel.resume_training: optimizers and schedulers from a `.state` file.  train.py:64-65 calls it right after
        build_model(), before any batch: the step (whose shapes come from the first batch) does not exist yet, so the state
        is kept and applied when it is built."""
        assert len(resume_state["optimizers"]) == 2, "Wrong lengths of optimizers"
        if self.ts is None:
            self._pending_state = resume_state
        else:
            self._apply_resume_state(resume_state)
        it = int(resume_state.get("iter", 0))
        if it > 0:   # the schedule is a function of the iteration: restore the LR the next update_learning_rate would continue from
            self.update_learning_rate(it)

    def _apply_resume_state(self, resume_state: dict):
        for o, s, name in zip((self.ts.opt_g, self.ts.opt_d), resume_state["optimizers"], ("optim_g", "optim_d")):
            slots = self._optimizer_slots(o)
            parts = getattr(o, "parts", (o,))        # (an optimizer over two arenas keeps one step counter per arena)
            per = s["state"]
            assert len(per) in (0, len(slots)), f"optimizer state has {len(per)} entries, network has {len(slots)} parameters"
            spec = o.spec if o.spec is not None else dict(optimizers.OPTIM_DEFAULTS["Adam"], type="Adam")
            optimizers.check_resume_type(name, spec, s)      # another optimizer type's state: refused by name
            if o.spec is not None:
                for i, (st, k, part) in enumerate(slots):
                    if i in per:
                        for a, t in part.arenas.items():
                            st.tensor(k, t).copy_(per[i][a].to(self.device, torch.float32))
                for part in parts:
                    part.step.fill_(optimizers.resumed_step(o.spec, s))
                continue
            step = 0
            for i, (st, k, part) in enumerate(slots):
                if i not in per:
                    continue
                e = per[i]
                st.tensor(k, part.exp_avg).copy_(e["exp_avg"].to(self.device, torch.float32))
                st.tensor(k, part.exp_avg_sq).copy_(e["exp_avg_sq"].to(self.device, torch.float32))
                step = int(float(e["step"]))
            for part in parts:
                part.step.fill_(step)
        self.ts.iter = int(resume_state.get("iter", 0))

    # ---- validation (ssr_esrgan_model.py:269-352; metrics: psnr / ssim as BasicSR, cpsnr as ssr/metrics/cpsnr.py, lpips as ssr/metrics/lpips.py) ----
    def validation(self, dataloader, current_iter, tb_logger, save_img=False):
        """BaseModel.validation -> nondist_validation on every rank's own loader (the reference's dist_validation only runs
        on rank 0)."""
        if self.dp is not None and self.dp.rank != 0:
            return
        self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        from .. import metrics as M
        ds_opt = getattr(getattr(dataloader, "dataset", None), "opt", None) or {}
        dataset_name = ds_opt.get("name", "val")
        sect = self.opt.get("test" if dataset_name == "test" else "val") or {}
        metrics2run = sect.get("metrics") or {}
        for name, mo in metrics2run.items():
            if mo.get("type") not in M.METRICS:
                raise NotImplementedError(f"metric {name}: type {mo.get('type')!r} is outside the MI355X path "
                                          f"(have {sorted(M.METRICS)})")
            if mo["type"] in M.METRIC_CHECKS:      # calculate_lpips: its keys and its weights file, before the first forward
                M.METRIC_CHECKS[mo["type"]](**{k: v for k, v in mo.items() if k not in ("type", "better")})
        self.metric_results = {m: 0.0 for m in metrics2run}
        rec = self.best_metric_results.setdefault(dataset_name, {})
        for m, mo in metrics2run.items():
            better = mo.get("better", "higher")
            rec.setdefault(m, dict(better=better, val=float("-inf") if better == "higher" else float("inf"), iter=-1))
        n = 0
        self._validating = True
        try:       # an exception below (bad image, unsupported metric option, OOM) must not leave the model in validation mode
            for idx, val_data in enumerate(dataloader):
                self.feed_data(val_data)
                self.test()
                # [B,H,W,3] uint8 RGB on the device (tensor2img: clamp, *255, round); raises instead of scoring NaN-derived pixels
                sr = M.tensor2img_u8(self.output, check_finite=True, compute_dtype=self.compute_dtype)
                gt = M.tensor2img_u8(self.gt) if self.gt is not None else None
                if save_img:
                    vis = self.opt.get("path", {}).get("visualization", "experiments/visualization")
                    base = os.path.join(vis, str(idx)) if self.opt.get("is_train", True) else os.path.join(vis, dataset_name)
                    os.makedirs(base, exist_ok=True)
                    tag = f"{idx}_{current_iter}" if self.opt.get("is_train", True) else f"{idx}_{self.opt.get('name', 'run')}"
                    M.imwrite_rgb(sr[0].cpu().numpy(), os.path.join(base, tag + ".png"))
                    if gt is not None:
                        M.imwrite_rgb(gt[0].cpu().numpy(), os.path.join(base, tag + "_gt.png"))
                if gt is not None:
                    for name, mo in metrics2run.items():
                        kw = {k: v for k, v in mo.items() if k not in ("type", "better")}
                        self.metric_results[name] += float(M.METRICS[mo["type"]](sr[:1], gt[:1], **kw))
                n += 1
                self.gt = self.output = None
        finally:
            self._validating = False
        for name in self.metric_results:
            self.metric_results[name] /= max(n, 1)
            r = rec[name]
            v = self.metric_results[name]
            if (r["better"] == "higher" and v >= r["val"]) or (r["better"] != "higher" and v <= r["val"]):
                r["val"], r["iter"] = v, current_iter
        if tb_logger is not None:
            for name, v in self.metric_results.items():
                tb_logger.add_scalar(f"metrics/{dataset_name}/{name}", v, current_iter)
        return self.metric_results
