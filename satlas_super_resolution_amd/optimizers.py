"""BasicSR's optimizers and learning-rate schedulers for the fused train step.

What BasicSR offers (`get_optimizer`: `torch.optim.<type>(params, lr, **kwargs)` from `train.optim_g` / `optim_d`; `setup_schedulers`:
MultiStepLR / MultiStepRestartLR / CosineAnnealingRestartLR from `train.scheduler`) and what the step runs on the device:

  * the update is one launch of csrc/optim.hip (ssr_optim_step[_guarded]) over the flat parameter arena - OptimState below, with
    the surface of train_step.AdamState (update / set_lr / ema / step / skipped / guard).  Plain Adam (weight_decay 0, no amsgrad)
    stays on AdamState and ssr_adam_step[_guarded]: the launches of a shipped option file do not change.
  * the arithmetic of every kind is torch.optim's single-tensor path (the DEFINITION; held to it in float64 by
    tests/test_gpu_optimizers.py).  Our own choices: grad_scale (the data-parallel 1/world) multiplies the gradient before weight
    decay; bias corrections are evaluated in fp32 on the device (as ssr_adam_step); SGD's "buffer does not exist yet" is the device
    counter of applied steps being 0, so a step skipped by the non-finite guard does not initialise it.
  * the schedules are closed forms in last_epoch = current_iter - 1, evaluated on the host (update_learning_rate).

BasicSR is not installed where this was written: what is stated from its source (basicsr/models/lr_scheduler.py, base_model.py) is
marked [recalled].  torch.optim is installed and was read."""
from __future__ import annotations

import ctypes as C
import math
from collections import Counter, OrderedDict
from typing import Dict, List, Optional, Sequence

import torch

from . import hip

# the numeric and boolean constructor arguments of torch.optim.<type> with their defaults (lr: BasicSR always passes it)
OPTIM_DEFAULTS: Dict[str, Dict] = {
    "Adam": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, decoupled_weight_decay=False),
    "AdamW": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False),
    "SGD": dict(lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False),
    "RMSprop": dict(lr=1e-2, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False),
}
# constructor arguments that select another implementation or another sign: refused by name
REFUSED_KEYS = ("maximize", "foreach", "capturable", "differentiable", "fused")
REFUSED_TYPES = ("Adamax", "ASGD", "Rprop")          # BasicSR's get_optimizer offers them; no kernel here
_BOOLS = ("amsgrad", "decoupled_weight_decay", "nesterov", "centered")


def normalize_optim(name: str, o: Optional[Dict]) -> Dict:
    """`train.<name>` (optim_g / optim_d) -> {"type", every constructor argument of OPTIM_DEFAULTS[type]}.  Unknown or unsupported
    types and keys raise NotImplementedError naming them; values torch's constructor rejects raise ValueError with its wording."""
    o = dict(o or {})
    typ = o.pop("type", "Adam")
    if typ in REFUSED_TYPES:
        raise NotImplementedError(f"train.{name}.type={typ!r}: no device kernel (have {', '.join(OPTIM_DEFAULTS)})")
    if typ not in OPTIM_DEFAULTS:
        raise NotImplementedError(f"train.{name}.type={typ!r}: only {', '.join(OPTIM_DEFAULTS)}")
    spec = dict(OPTIM_DEFAULTS[typ])
    for k, v in o.items():
        if k in REFUSED_KEYS:
            if v in (None, False):          # the constructor's own default: nothing is asked for
                continue
            raise NotImplementedError(f"train.{name}.{k}: not supported on the device path")
        if k not in spec:
            raise NotImplementedError(f"train.{name}.{k}: torch.optim.{typ} takes {', '.join(spec)}")
        if k == "betas":
            if not (isinstance(v, (list, tuple)) and len(v) == 2):
                raise ValueError(f"train.{name}.betas={v!r}: two numbers")
            spec[k] = (float(v[0]), float(v[1]))
        elif k in _BOOLS:
            if not isinstance(v, bool):
                raise ValueError(f"train.{name}.{k}={v!r}: a boolean")
            spec[k] = v
        else:
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"train.{name}.{k}={v!r}: a number")
            spec[k] = float(v)
    # torch's own constructor checks, in its words
    if not 0.0 <= spec["lr"]:
        raise ValueError(f"train.{name}.lr: Invalid learning rate: {spec['lr']}")
    if not 0.0 <= spec["weight_decay"]:
        raise ValueError(f"train.{name}.weight_decay: Invalid weight_decay value: {spec['weight_decay']}")
    if "eps" in spec and not 0.0 <= spec["eps"]:
        raise ValueError(f"train.{name}.eps: Invalid epsilon value: {spec['eps']}")
    if "betas" in spec:
        for i, b in enumerate(spec["betas"]):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"train.{name}.betas: Invalid beta parameter at index {i}: {b}")
    if "momentum" in spec and not 0.0 <= spec["momentum"]:
        raise ValueError(f"train.{name}.momentum: Invalid momentum value: {spec['momentum']}")
    if "alpha" in spec and not 0.0 <= spec["alpha"]:
        raise ValueError(f"train.{name}.alpha: Invalid alpha value: {spec['alpha']}")
    if spec.get("nesterov") and (spec["momentum"] <= 0 or spec["dampening"] != 0):
        raise ValueError(f"train.{name}.nesterov: Nesterov momentum requires a momentum and zero dampening")
    spec["type"] = typ
    return spec


def is_plain_adam(spec: Optional[Dict]) -> bool:
    """what ssr_adam_step computes: Adam, no weight decay, no amsgrad"""
    return spec is None or (spec["type"] == "Adam" and spec["weight_decay"] == 0.0 and not spec["amsgrad"])


def state_keys(spec: Dict) -> List[str]:
    """torch's per-parameter state tensors of this optimizer, in the order its state dict holds them (besides 'step')"""
    t = spec["type"]
    if t in ("Adam", "AdamW"):
        return ["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if spec["amsgrad"] else [])
    if t == "SGD":
        return ["momentum_buffer"] if spec["momentum"] != 0 else []
    return ["square_avg"] + (["momentum_buffer"] if spec["momentum"] > 0 else []) + (["grad_avg"] if spec["centered"] else [])


def has_step(spec: Dict) -> bool:
    return spec["type"] != "SGD"          # torch.optim.SGD keeps no 'step'


def kernel_kind(spec: Dict) -> int:
    if spec["type"] == "Adam" and spec.get("decoupled_weight_decay"):     # torch.optim.AdamW is Adam(decoupled_weight_decay=True)
        return hip.OPTIM_KINDS["AdamW"]
    return hip.OPTIM_KINDS[spec["type"]]


def kernel_flags(spec: Dict) -> int:
    return (hip.OPT_AMSGRAD if spec.get("amsgrad") else 0) | (hip.OPT_NESTEROV if spec.get("nesterov") else 0) | \
        (hip.OPT_CENTERED if spec.get("centered") else 0)


def optim_args(spec: Dict, ptrs: Dict[str, Optional[int]], n: int, ema_decay: float = 0.0, grad_scale: float = 1.0) -> "hip.OptimArgs":
    """ssr_optim_args of `spec` over the device addresses in `ptrs` (param, grad, lr, step, ema and the state_keys(spec))"""
    betas = spec.get("betas", (0.0, 0.0))
    return hip.OptimArgs(ptrs["param"], ptrs["grad"], ptrs.get("exp_avg"), ptrs.get("exp_avg_sq"), ptrs.get("max_exp_avg_sq"),
                         ptrs.get("momentum_buffer"), ptrs.get("square_avg"), ptrs.get("grad_avg"), ptrs.get("ema"), n,
                         ptrs["lr"], ptrs["step"], kernel_kind(spec), kernel_flags(spec), betas[0], betas[1],
                         spec.get("eps", 0.0), spec["weight_decay"], spec.get("momentum", 0.0), spec.get("dampening", 0.0),
                         spec.get("alpha", 0.0), ema_decay, grad_scale)


class OptimState:
    """torch.optim.<spec type> state over a ParamStore's flat arena (+ optional EMA arena): train_step.AdamState for the other
    optimizers.  `arenas` holds one flat fp32 tensor per torch state key that the options need (state_keys), nothing else.

    guard: as AdamState - update() scans the gradient arena for NaN / +-Inf into `flag`, the guarded launch then skips a flagged step on
    the device (parameters, every arena and `step` stay; the EMA still moves), counts it in `skipped` and clears the flag."""

    def __init__(self, store, spec: Dict, ema_decay: float = 0.0, guard: bool = True):
        dev = store.device
        self.store, self.spec = store, dict(spec)
        self.arenas = OrderedDict((k, torch.zeros_like(store.data)) for k in state_keys(spec))
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)          # applied steps
        self.lr = torch.full((1,), spec["lr"], dtype=torch.float32, device=dev)
        self.ema = store.data.clone() if ema_decay > 0 else None
        ptrs = {k: t.data_ptr() for k, t in self.arenas.items()}
        ptrs.update(param=store.data.data_ptr(), grad=store.grad.data_ptr(), lr=self.lr.data_ptr(), step=self.step.data_ptr(),
                    ema=self.ema.data_ptr() if self.ema is not None else None)
        self.args = optim_args(spec, ptrs, store.numel, ema_decay)
        self.guard = guard
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.skipped = torch.zeros(1, dtype=torch.int32, device=dev)
        self._scan_src = (C.c_void_p * 1)(store.grad.data_ptr())
        self._scan_n = (C.c_int64 * 1)(store.numel)

    def set_lr(self, lr: float):
        self.lr.fill_(lr)

    def update(self, grad_scale: float = 1.0):
        self.args.grad_scale = grad_scale
        L, st = hip.lib(), hip.stream_ptr()
        if not self.guard:
            hip.check(L.ssr_optim_step(C.byref(self.args), st), "ssr_optim_step")
            return
        hip.check(L.ssr_nonfinite_scan(self._scan_src, self._scan_n, 1, self.flag.data_ptr(), st), "ssr_nonfinite_scan")
        hip.check(L.ssr_optim_step_guarded(C.byref(self.args), self.flag.data_ptr(), self.skipped.data_ptr(), st),
                  "ssr_optim_step_guarded")


# ------------------------------------------------------------------------------------------------ checkpoints
def param_group(spec: Dict, lr: float, n_params: int) -> Dict:
    """the param group torch.optim.<type>(params, **spec).state_dict() holds - taken from the installed class itself, so the keys are
    this torch's - with the scheduled `lr` and BasicSR's `initial_lr` (the scheduler's constructor adds it)"""
    kw = {k: v for k, v in spec.items() if k != "type"}
    g = getattr(torch.optim, spec["type"])([torch.nn.Parameter(torch.zeros(1))], **kw).state_dict()["param_groups"][0]
    g["lr"], g["initial_lr"], g["params"] = lr, spec["lr"], list(range(n_params))
    return g


def optimizer_state_dict(spec: Dict, lr: float, per_param: Sequence[Dict[str, torch.Tensor]], step: int) -> Dict:
    """torch.optim.<type>.state_dict() over parameters in named_parameters() order.  per_param[i]: {state key: tensor shaped like
    parameter i} for the keys of state_keys(spec).  As in torch, state appears with the first applied step (`step` > 0) and 'step' is
    a float32 scalar tensor where the optimizer keeps one (not SGD)."""
    keys = state_keys(spec)
    state = {}
    if step > 0 and (keys or has_step(spec)):
        for i, tensors in enumerate(per_param):
            e = {"step": torch.tensor(float(step))} if has_step(spec) else {}
            for k in keys:
                e[k] = tensors[k].detach().cpu().clone()
            state[i] = e
    return {"state": state, "param_groups": [param_group(spec, lr, len(per_param))]}


def state_dict_type(sd: Dict) -> str:
    """which torch.optim class wrote this state dict, from its param group's keys ('Adam/AdamW' where an older torch's group does
    not say which)"""
    g = sd["param_groups"][0]
    if "betas" in g:
        if "decoupled_weight_decay" not in g:
            return "Adam/AdamW"
        return "AdamW" if g["decoupled_weight_decay"] else "Adam"
    if "alpha" in g and "centered" in g:
        return "RMSprop"
    if "nesterov" in g:
        return "SGD"
    return "unknown"


def check_resume_type(name: str, spec: Dict, sd: Dict):
    """a `.state` written by one optimizer type and resumed under another is refused by name"""
    wrote = state_dict_type(sd)
    mine = "AdamW" if kernel_kind(spec) == hip.OPTIM_KINDS["AdamW"] else spec["type"]
    if wrote != mine and not (wrote == "Adam/AdamW" and mine in ("Adam", "AdamW")):
        raise ValueError(f"resume: the state of {name} was written by torch.optim.{wrote}, the option file asks for {mine}")
    for i, e in sd["state"].items():
        for k in state_keys(spec):
            if k not in e or e[k] is None:
                raise ValueError(f"resume: the state of {name} (parameter {i}) has no {k!r}, which {mine} with these options needs")
        break


def resumed_step(spec: Dict, sd: Dict) -> int:
    """the applied-step counter a state dict stands for.  SGD keeps no 'step': a present momentum_buffer means initialised (only
    zero / non-zero matters to the kernel)"""
    for e in sd["state"].values():
        if "step" in e:
            return int(float(e["step"]))
        return 1 if e.get("momentum_buffer") is not None else 0
    return 0


# ------------------------------------------------------------------------------------------------ schedules
def multistep_restart_lr(base: float, last_epoch: int, milestones: Sequence[int], gamma: float,
                         restarts: Sequence[int] = (0,), restart_weights: Sequence[float] = (1,)) -> float:
    """MultiStepLR / BasicSR MultiStepRestartLR in closed form: base * w_r * gamma^k with r the latest restart <= last_epoch (none yet:
    weight 1, counting from the start) and k the milestones, with multiplicity, in (r, last_epoch].

    [recalled] basicsr MultiStepRestartLR.get_lr chains: at a restart lr = initial_lr * weight (this wins over a milestone at the same
    epoch), at a milestone lr *= gamma ** multiplicity, otherwise unchanged."""
    r, w = -1, 1.0
    for e, we in zip(restarts, restart_weights):
        if r < e <= last_epoch:
            r, w = e, we
    k = sum(1 for m in milestones if r < m <= last_epoch) if r >= 0 else sum(1 for m in milestones if m <= last_epoch)
    return base * (w * gamma ** k)


def cosine_restart_lr(base: float, last_epoch: int, periods: Sequence[int], restart_weights: Sequence[float] = (1,),
                      eta_min: float = 0.0) -> float:
    """[recalled] basicsr CosineAnnealingRestartLR.get_lr, which is a closed form already: idx = the first i with
    last_epoch <= cumsum(periods)[i]; lr = eta_min + w_idx * 0.5 * (base - eta_min) * (1 + cos(pi * (last_epoch - start_idx) /
    periods[idx])), start_idx = the previous cumulative period.  Past the last period BasicSR's index lookup fails: IndexError."""
    cum, start = 0, 0
    for idx, p in enumerate(periods):
        start, cum = cum, cum + p
        if last_epoch <= cum:
            return eta_min + restart_weights[idx] * 0.5 * (base - eta_min) * (1 + math.cos(math.pi * ((last_epoch - start) / p)))
    raise IndexError(f"train.scheduler CosineAnnealingRestartLR: iteration {last_epoch + 1} is past the last period "
                     f"(periods sum to {cum})")


class Schedule:
    """`train.scheduler` validated: lr(base, current_iter, warmup_iter) on the host, state_dict(...) in BasicSR's layout."""

    def __init__(self, sch: Optional[Dict], total_iter: Optional[int] = None):
        sch = dict(sch or {})
        self.type = sch.pop("type", "MultiStepLR") if sch else None
        if self.type in (None, "MultiStepLR", "MultiStepRestartLR"):
            self.milestones = [int(m) for m in sch.pop("milestones", [])]
            self.gamma = float(sch.pop("gamma", 0.1)) if self.type else 1.0
            self.restarts = [int(r) for r in sch.pop("restarts", [0])]
            self.restart_weights = [float(w) for w in sch.pop("restart_weights", [1])]
            if len(self.restarts) != len(self.restart_weights):
                raise ValueError("train.scheduler: restarts and restart_weights should have the same length")
        elif self.type == "CosineAnnealingRestartLR":
            if "periods" not in sch:
                raise ValueError("train.scheduler.periods: CosineAnnealingRestartLR needs it")
            self.periods = [int(p) for p in sch.pop("periods")]
            self.restart_weights = [float(w) for w in sch.pop("restart_weights", [1])]
            self.eta_min = float(sch.pop("eta_min", 0))
            if len(self.periods) != len(self.restart_weights) or not self.periods or min(self.periods) <= 0:
                raise ValueError("train.scheduler: periods (positive) and restart_weights should have the same length")
            if total_iter is not None and int(total_iter) - 1 > sum(self.periods):
                raise ValueError(f"train.scheduler.periods sum to {sum(self.periods)}, train.total_iter is {int(total_iter)}: the schedule "
                                 "ends before the training does")
        else:
            raise NotImplementedError(f"train.scheduler.type={self.type!r}: only MultiStepLR, MultiStepRestartLR, CosineAnnealingRestartLR")
        for k in sch:
            raise NotImplementedError(f"train.scheduler.{k}: {self.type} does not take it")

    @property
    def plain_multistep(self) -> bool:
        return self.type != "CosineAnnealingRestartLR" and self.restarts == [0] and self.restart_weights == [1.0]

    def lr(self, base: float, current_iter: int, warmup_iter: int = -1) -> float:
        """BasicSR BaseModel.update_learning_rate: the scheduler is stepped once per call from the second call on
        (last_epoch = current_iter - 1); during warm-up the LR is base * current_iter / warmup_iter."""
        if warmup_iter > 0 and current_iter < warmup_iter:
            return base * (current_iter / warmup_iter)
        last = current_iter - 1
        if self.type == "CosineAnnealingRestartLR":
            return cosine_restart_lr(base, max(last, 0), self.periods, self.restart_weights, self.eta_min)
        return multistep_restart_lr(base, last, self.milestones, self.gamma, self.restarts, self.restart_weights)

    def state_dict(self, base_lr: float, lr: float, current_iter: int) -> Dict:
        """[recalled] the BasicSR scheduler's __dict__ minus the optimizer (torch LRScheduler.state_dict)"""
        last = max(int(current_iter) - 1, 0)
        common = {"base_lrs": [base_lr], "last_epoch": last, "_step_count": last + 1, "verbose": False,
                  "_get_lr_called_within_step": False, "_last_lr": [lr]}
        if self.type == "CosineAnnealingRestartLR":
            cum = [sum(self.periods[:i + 1]) for i in range(len(self.periods))]
            return {"periods": list(self.periods), "restart_weights": list(self.restart_weights), "eta_min": self.eta_min,
                    "cumulative_period": cum, **common}
        plain = self.plain_multistep
        return {"milestones": Counter(self.milestones), "gamma": self.gamma, "restarts": [0] if plain else list(self.restarts),
                "restart_weights": [1] if plain else list(self.restart_weights), **common}
