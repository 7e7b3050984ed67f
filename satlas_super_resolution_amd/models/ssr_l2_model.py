"""L2Model on MI355X - the model plugin that trains and evaluates the reference's two comparison baselines, SRCNN and HighResNet
(ssr/models/ssr_l2_model.py; option files srcnn_s2naip_urban.yml and highresnet_s2naip_urban.yml).  Same registry name, the same `opt`
keys, driven by train.py and test.py unchanged:

    feed_data(:25-28)  optimize_parameters(:30-54)  test(:56-60)  get_current_visuals(:62-68)  nondist_validation(:85-159)
    + the BasicSR BaseModel methods train.py calls: update_learning_rate, get_current_learning_rate, get_current_log, save,
      resume_training, validation.

The step: forward in training mode (archs/l2_archs.py), the hard-coded loss 0.3 mse + 0.4 mae + 0.3 ssim (ssr_mse_l1_loss, then
ssr_ssim_loss accumulating into the same gradient; the reference's batch mean of per-sample means is the plain mean), backward, and
the `optim_g` update through optimizers.OptimState - every kind it offers, with the non-finite guard of the ESRGAN step.  The launches
are issued eagerly, not captured into a hipGraph ("L2Model").  Deterministic throughout: no float atomics.

`train.pixel_opt` is accepted and IGNORED, as in the reference (its loss is hard-coded; the shipped option files carry an L1Loss block
that SRModel builds and L2Model never calls).  No discriminator.  EMA runs only if train.ema_decay > 0 (SRModel's rule [recalled]).
Data-parallel training (world size > 1) raises NotImplementedError.  test() hands a [B, 1, 3, 4H, 4W] tensor on, which BasicSR's
tensor2img rejects in the reference; here validation squeezes the revisit axis.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict

import torch

from .. import hip, optimizers
from ..hip import view
from ..l2_reference import W_MAE, W_MSE, W_SSIM
from ..registry import MODEL_REGISTRY, build_network

ARCHS = ("SRCNN", "HighResNet")


def network_from_opt(opt: dict):
    """validates `network_g` (and `compute_dtype`) and builds the arch; everything unsupported raises NotImplementedError by name"""
    from ..archs import l2_archs  # noqa: F401  (registers SRCNN / HighResNet)
    net_opt = dict(opt["network_g"])
    if net_opt.get("type") not in ARCHS:
        raise NotImplementedError(f"network_g.type={net_opt.get('type')!r}: L2Model drives {' / '.join(ARCHS)}")
    net_opt.setdefault("compute_dtype", opt.get("compute_dtype", "fp32"))
    return build_network(net_opt)


def validate_options(opt: dict):
    """Everything L2Model reads from an option file, checked without a GPU: returns (network on the CPU, optimizer spec or None,
    schedule, ema_decay).  The network is initialised under a forked RNG seeded with manual_seed: the caller's global stream (the
    dataloaders') is left untouched."""
    is_train = opt.get("is_train", True)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if is_train and (world > 1 or (opt.get("dist", False) and int(opt.get("world_size", world)) > 1)):
        raise NotImplementedError("L2Model: data-parallel training (world_size > 1) is outside this path; run it on one GPU")
    train_opt = opt.get("train", {}) or {}
    spec = optimizers.normalize_optim("optim_g", train_opt.get("optim_g")) if is_train else None
    schedule = optimizers.Schedule(train_opt.get("scheduler"), train_opt.get("total_iter") if is_train else None)
    with torch.random.fork_rng(devices=[]):
        if opt.get("manual_seed") is not None:
            torch.manual_seed(int(opt["manual_seed"]))
        net = network_from_opt(opt)
    return net, spec, schedule, float(train_opt.get("ema_decay", 0) or 0)


@MODEL_REGISTRY.register()
class L2Model:
    def __init__(self, opt: dict):
        self.opt = opt
        self.is_train = opt.get("is_train", True)
        self.net_g, self.spec, self.schedule, self.ema_decay = validate_options(opt)      # option errors surface before the GPU is needed
        if not torch.cuda.is_available():
            raise hip.HipLibraryError("L2Model needs an MI355X (no CPU fallback; the CPU statement is l2_reference.py)")
        hip.lib()
        self.device = torch.device("cuda")
        path = opt.get("path", {}) or {}
        ema_sd = None
        if path.get("pretrain_network_g"):
            ck = torch.load(path["pretrain_network_g"], map_location="cpu")
            self.net_g.load_state_dict(ck[path.get("param_key_g", "params")], strict=path.get("strict_load_g", True))
            ema_sd = ck.get("params_ema")
        self.net_g.to(self.device)
        self.net_g.manual_seed(int(opt.get("manual_seed") or 0))
        self.store = self.net_g.store()
        self.net_g.train(self.is_train)
        self.opt_g = None
        if self.is_train:
            self.opt_g = optimizers.OptimState(self.store.live_view(), self.spec, ema_decay=self.ema_decay, guard=True)
            if ema_sd is not None and self.opt_g.ema is not None:
                for k in self.store.live_keys:
                    self.store.tensor(k, self.opt_g.ema).copy_(ema_sd[k].to(self.device, torch.float32))
        self.base_lr = self.spec["lr"] if self.is_train else 0.0
        self.current_lr = self.base_lr
        self.iter = 0
        self._loss = torch.zeros(4, dtype=torch.float32, device=self.device)          # mse, mae, 0.3 * ssim slot sum, spare
        self._ssim_slots = torch.zeros(hip.LOSS_SLOTS, dtype=torch.float32, device=self.device)
        self._partial = torch.zeros(2 * hip.L2_SLOTS, dtype=torch.float64, device=self.device)
        self._gt_buf = None
        self.log_dict = OrderedDict()
        self.lr = self.gt = self.output = None
        self.metric_results = {}
        self.best_metric_results = {}

    # ---- the methods train.py calls ----
    @torch.no_grad()
    def feed_data(self, data: dict):
        """ssr_l2_model.py:25-28: lr [B, n, C, h, w] and hr [B, C, 4h, 4w], uint8-valued -> float / 255"""
        self.lr = data["lr"].to(self.device).float() / 255
        if self.lr.dim() != 5:
            raise ValueError(f"L2Model: lr of shape {tuple(self.lr.shape)}; the dataset must stack revisits (use_3d: True) to [B, n, C, h, w]")
        self.gt = data["hr"].to(self.device).float() / 255 if "hr" in data else None

    def _loss_and_grad(self, plan, with_grad: bool = True):
        B, C, Ho, Wo = self.gt.shape
        L, st = hip.lib(), hip.stream_ptr()
        if self._gt_buf is None or self._gt_buf.shape[:3] != (B, Ho, Wo):
            self._gt_buf = torch.zeros(B, Ho, Wo, 8, dtype=torch.float32, device=self.device)
        gt = self.gt.contiguous()
        hip.check(L.ssr_nchw_to_nhwc(gt.data_ptr(), B, C, Ho, Wo, view(self._gt_buf), hip.F32, 1, 1, 1.0, st), "ssr_nchw_to_nhwc")
        self._loss.zero_()
        self._ssim_slots.zero_()
        grad = view(plan.d_out) if with_grad else hip.NULL_VIEW
        hip.check(L.ssr_mse_l1_loss(view(plan.out), view(self._gt_buf), grad, B * Ho * Wo, C, W_MSE, W_MAE, self._loss.data_ptr(),
                                    self._partial.data_ptr(), st), "ssr_mse_l1_loss")
        hip.check(L.ssr_ssim_loss(view(plan.out), view(self._gt_buf), grad, hip.F32 | hip.DETERMINISTIC, B, Ho, Wo, C, W_SSIM, 1,
                                  self._ssim_slots.data_ptr(), st), "ssr_ssim_loss")

    def optimize_parameters(self, current_iter: int, dropout_masks=None):
        net, stg = self.net_g, self.store
        net.train()
        net.check_input(self.lr)
        B, R, C, H, W = self.lr.shape
        plan = net.plan(B, H, W, True)
        with torch.no_grad():
            net._run(plan, self.lr, dropout_masks)
        self.plan = plan
        self._loss_and_grad(plan)
        stg.grad.zero_()
        plan.bwd.run()
        self.opt_g.update()
        self.iter += 1
        self.output = None

    def get_current_log(self):
        mse, mae = (float(v) for v in self._loss[:2].tolist())
        ssim = float(self._ssim_slots.double().sum().item()) / W_SSIM      # the slots hold weight * mean, added here in index order
        self.log_dict = OrderedDict(psnr_loss=10.0 * math.log10(mse) if mse > 0 else float("-inf"), mse=mse, mae=mae, ssim=ssim,
                                    tot_loss=W_MSE * mse + W_MAE * mae + W_SSIM * ssim)
        return self.log_dict

    @property
    def nonfinite_skips(self) -> dict:
        return {"net_g": int(self.opt_g.skipped.item()) if self.opt_g is not None else 0, "net_d": 0}

    def update_learning_rate(self, current_iter: int, warmup_iter: int = -1):
        self.current_lr = self.schedule.lr(self.base_lr, current_iter, warmup_iter)
        if self.opt_g is not None:
            self.opt_g.set_lr(self.current_lr)

    def get_current_learning_rate(self):
        return [self.current_lr]

    def test(self):
        """:56-60 - eval mode (Dropout off), no grad; with the EMA weights when train.ema_decay > 0 (SRModel.test [recalled])"""
        net = self.net_g
        saved = None
        if self.opt_g is not None and self.opt_g.ema is not None:
            n = self.store.live_numel
            saved = self.store.data[:n].clone()
            self.store.data[:n].copy_(self.opt_g.ema)
        net.eval()
        try:
            with torch.no_grad():
                self.output = net(self.lr)
        finally:
            net.train(self.is_train)
            if saved is not None:
                self.store.data[:self.store.live_numel].copy_(saved)

    def get_current_visuals(self):
        out = OrderedDict()
        out["lr"] = self.lr.detach().cpu()
        res = self.output if self.output is not None else self.plan.read_output()[:, None]
        out["result"] = res.detach().cpu()
        if self.gt is not None:
            out["gt"] = self.gt.detach().cpu()
        return out

    # ---- checkpoints (BasicSR layout) ----
    def state_dict(self, ema: bool = False) -> "OrderedDict[str, torch.Tensor]":
        sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in self.net_g.state_dict().items())
        if ema:
            names = dict(self.net_g.named_parameters())
            by_id = {id(p): k for k, p in names.items()}
            live = set(self.store.live_keys)
            full = dict(self.net_g.named_parameters(remove_duplicate=False))
            for k in sd:
                canon = by_id[id(full[k])]
                if canon in live:
                    sd[k] = self.store.tensor(canon, self.opt_g.ema).detach().cpu().clone()
        return sd

    def save(self, epoch: int, current_iter: int):
        it = "latest" if current_iter == -1 else str(current_iter)
        path = self.opt.get("path", {}) or {}
        mdir, sdir = path.get("models", "experiments/models"), path.get("training_states", "experiments/training_states")
        os.makedirs(mdir, exist_ok=True)
        os.makedirs(sdir, exist_ok=True)
        g = {"params": self.state_dict()}
        if self.opt_g is not None and self.opt_g.ema is not None:
            g["params_ema"] = self.state_dict(ema=True)
        torch.save(g, os.path.join(mdir, f"net_g_{it}.pth"))
        if self.opt_g is None:
            return
        o, stg = self.opt_g, self.store
        live = set(stg.live_keys)
        # torch keeps optimizer state only for parameters that received a gradient: the dead ones have an (empty-handed) index
        per = [({a: stg.tensor(k, t) for a, t in o.arenas.items()} if k in live else None) for k in stg.keys]
        osd = optimizers.optimizer_state_dict(self.spec, self.current_lr, [p or {a: torch.zeros(0) for a in o.arenas} for p in per],
                                              int(o.step.item()))
        for i, p in enumerate(per):
            if p is None:
                osd["state"].pop(i, None)
        state = {"epoch": epoch, "iter": current_iter, "optimizers": [osd],
                 "schedulers": [self.schedule.state_dict(self.base_lr, self.current_lr, current_iter)],
                 "dropout_step": int(self.net_g.drop_step.item())}
        torch.save(state, os.path.join(sdir, f"{it}.state"))

    def resume_training(self, resume_state: dict):
        """BaseModel.resume_training: optimizer state, LR schedule position and the dropout generator's step counter (ours: BasicSR's
        files do not carry one; without the key the counter continues from the resumed iteration)"""
        assert len(resume_state["optimizers"]) == 1, "Wrong lengths of optimizers"
        s, o, stg = resume_state["optimizers"][0], self.opt_g, self.store
        optimizers.check_resume_type("optim_g", self.spec, s)
        for i, k in enumerate(stg.keys):
            if i in s["state"] and k in stg.live_keys:
                for a, t in o.arenas.items():
                    stg.tensor(k, t).copy_(s["state"][i][a].to(self.device, torch.float32))
        o.step.fill_(optimizers.resumed_step(self.spec, s))
        it = int(resume_state.get("iter", 0))
        self.iter = it
        self.net_g.drop_step.fill_(int(resume_state.get("dropout_step", it)))
        if it > 0:
            self.update_learning_rate(it)

    # ---- validation (psnr / ssim / cpsnr / lpips on the device, as SSRESRGANModel) ----
    def validation(self, dataloader, current_iter, tb_logger, save_img=False):
        self.nondist_validation(dataloader, current_iter, tb_logger, save_img)

    def nondist_validation(self, dataloader, current_iter, tb_logger, save_img):
        from .. import metrics as M
        ds_opt = getattr(getattr(dataloader, "dataset", None), "opt", None) or {}
        dataset_name = ds_opt.get("name", "val")
        sect = self.opt.get("test" if dataset_name == "test" else "val") or {}
        metrics2run = sect.get("metrics") or {}
        for name, mo in metrics2run.items():
            if mo.get("type") not in M.METRICS:
                raise NotImplementedError(f"metric {name}: type {mo.get('type')!r} is outside the MI355X path (have {sorted(M.METRICS)})")
            if mo["type"] in M.METRIC_CHECKS:
                M.METRIC_CHECKS[mo["type"]](**{k: v for k, v in mo.items() if k not in ("type", "better")})
        self.metric_results = {m: 0.0 for m in metrics2run}
        rec = self.best_metric_results.setdefault(dataset_name, {})
        for m, mo in metrics2run.items():
            better = mo.get("better", "higher")
            rec.setdefault(m, dict(better=better, val=float("-inf") if better == "higher" else float("inf"), iter=-1))
        n = 0
        for idx, val_data in enumerate(dataloader):
            self.feed_data(val_data)
            self.test()
            # the reference passes the 5-D [B, 1, C, 4h, 4w] result to tensor2img, which BasicSR rejects: squeeze the revisit axis
            sr = M.tensor2img_u8(self.output.squeeze(1).contiguous(), check_finite=True, compute_dtype="fp32")
            gt = M.tensor2img_u8(self.gt) if self.gt is not None else None
            if save_img:
                vis = (self.opt.get("path", {}) or {}).get("visualization", "experiments/visualization")
                base = os.path.join(vis, str(idx)) if self.opt.get("is_train", True) else os.path.join(vis, dataset_name)
                os.makedirs(base, exist_ok=True)
                tag = f"{idx}_{current_iter}" if self.opt.get("is_train", True) else f"{idx}_{self.opt.get('name', 'run')}"
                M.imwrite_rgb(sr[0].cpu().numpy(), os.path.join(base, tag + ".png"))
            if gt is not None:
                for name, mo in metrics2run.items():
                    kw = {k: v for k, v in mo.items() if k not in ("type", "better")}
                    self.metric_results[name] += float(M.METRICS[mo["type"]](sr[:1], gt[:1], **kw))
            n += 1
            self.gt = self.output = None
        for name in self.metric_results:
            self.metric_results[name] /= max(n, 1)
            r, v = rec[name], self.metric_results[name]
            if (r["better"] == "higher" and v >= r["val"]) or (r["better"] != "higher" and v <= r["val"]):
                r["val"], r["iter"] = v, current_iter
        if tb_logger is not None:
            for name, v in self.metric_results.items():
                tb_logger.add_scalar(f"metrics/{dataset_name}/{name}", v, current_iter)
        return self.metric_results
