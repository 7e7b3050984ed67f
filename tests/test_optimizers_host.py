"""CPU: the host side of BasicSR's other optimizers and schedulers - option parsing (train_config_from_opt, optimizers.normalize_optim),
the closed-form schedules (optimizers.multistep_restart_lr / cosine_restart_lr / Schedule) and the checkpoint layout
(optimizers.optimizer_state_dict, the function SSRESRGANModel.save calls) against the installed torch.optim."""
import copy
import inspect
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN


def _shipped():
    return json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]


def _with(opt, name, block):
    o = copy.deepcopy(opt)
    o["train"][name] = block
    return o


# ================================================================================================ option parsing
def test_adamw_with_weight_decay_on_the_shipped_option_file_returns_a_config():
    """the case that raised before the feature: esrgan_s2naip_urban.yml with optim_g.type AdamW, weight_decay 0.01"""
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = _shipped()
    opt["train"]["optim_g"].update(type="AdamW", weight_decay=0.01)
    cfg = train_config_from_opt(opt)
    assert cfg.optim_g["type"] == "AdamW" and cfg.optim_g["weight_decay"] == 0.01 and cfg.optim_g["amsgrad"] is False
    assert cfg.optim_g["lr"] == cfg.lr_g == 1e-4 and cfg.optim_g["betas"] == (0.9, 0.99)
    assert cfg.optim_d is None                         # optim_d is the file's plain Adam: the launches it always had


def test_shipped_option_file_keeps_the_plain_adam_path():
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt, train_config_from_opt
    opt = _shipped()
    cfg = train_config_from_opt(opt)
    assert cfg.optim_g is None and cfg.optim_d is None
    ref = step_config_from_opt(opt)
    assert (cfg.lr_g, cfg.lr_d, cfg.betas, cfg.betas_d, cfg.eps) == (ref.lr_g, ref.lr_d, ref.betas, ref.betas_d, ref.eps)


def test_accepted_keys_are_the_torch_constructors_numeric_and_boolean_arguments():
    """OPTIM_DEFAULTS against inspect.signature of the installed classes: every argument but `params` and the refused ones, with
    torch's defaults"""
    from satlas_super_resolution_amd import optimizers as O
    for typ, defaults in O.OPTIM_DEFAULTS.items():
        sig = inspect.signature(getattr(torch.optim, typ).__init__).parameters
        takes = {k: p.default for k, p in sig.items() if k not in ("self", "params") + O.REFUSED_KEYS}
        assert set(takes) == set(defaults), (typ, set(takes) ^ set(defaults))
        for k, v in takes.items():
            assert defaults[k] == v and type(defaults[k]) in (type(v), float), (typ, k, v, defaults[k])


ACCEPTED = [
    ("Adam", dict(lr=2e-4, betas=[0.8, 0.95], eps=1e-6, weight_decay=0.02, amsgrad=True)),
    ("Adam", dict(lr=2e-4, weight_decay=0.02, decoupled_weight_decay=True)),
    ("AdamW", dict(lr=3e-4, betas=[0.5, 0.9], eps=1e-7, weight_decay=0.05, amsgrad=True)),
    ("SGD", dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=1e-4, nesterov=False)),
    ("SGD", dict(lr=1e-2, momentum=0.9, nesterov=True)),
    ("RMSprop", dict(lr=5e-5, alpha=0.9, eps=1e-6, weight_decay=1e-3, momentum=0.5, centered=True)),
]


@pytest.mark.parametrize("typ,kw", ACCEPTED, ids=[f"{t}-{i}" for i, (t, _) in enumerate(ACCEPTED)])
@pytest.mark.parametrize("name", ["optim_g", "optim_d"])
def test_each_accepted_type_and_key_lands_in_the_config(name, typ, kw):
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    cfg = train_config_from_opt(_with(_shipped(), name, dict(kw, type=typ)))
    spec = getattr(cfg, name)
    assert spec["type"] == typ
    for k, v in kw.items():
        assert spec[k] == (tuple(v) if k == "betas" else v), (k, spec[k])
    for k, v in O.OPTIM_DEFAULTS[typ].items():          # what the block leaves out: torch's default
        if k not in kw:
            assert spec[k] == v
    assert (cfg.lr_g if name == "optim_g" else cfg.lr_d) == kw["lr"]
    other = "optim_d" if name == "optim_g" else "optim_g"
    assert getattr(cfg, other) is None                  # G and D are described independently
    # the installed class takes exactly this description
    getattr(torch.optim, typ)([torch.nn.Parameter(torch.zeros(2))], **{k: v for k, v in spec.items() if k != "type"})


REFUSED = [(dict(type="Adam", maximize=True), NotImplementedError, "maximize"), (dict(type="AdamW", foreach=True), NotImplementedError, "foreach"),
           (dict(type="RMSprop", capturable=True), NotImplementedError, "capturable"),
           (dict(type="SGD", differentiable=True), NotImplementedError, "differentiable"), (dict(type="Adam", fused=True), NotImplementedError, "fused"),
           (dict(type="Adam", momentum=0.9), NotImplementedError, "momentum"), (dict(type="SGD", betas=[0.9, 0.99]), NotImplementedError, "betas"),
           (dict(type="RMSprop", nesterov=True), NotImplementedError, "nesterov"), (dict(type="AdamW", decoupled_weight_decay=True), NotImplementedError, "decoupled_weight_decay"),
           (dict(type="Adam", clip_grad=1.0), NotImplementedError, "clip_grad"),
           (dict(type="Adamax"), NotImplementedError, "Adamax"), (dict(type="ASGD"), NotImplementedError, "ASGD"), (dict(type="Rprop"), NotImplementedError, "Rprop"),
           (dict(type="Lion"), NotImplementedError, "Lion"),
           # invalid combinations and values: torch's constructor raises ValueError for each of these
           (dict(type="SGD", nesterov=True), ValueError, "nesterov"), (dict(type="SGD", nesterov=True, momentum=0.9, dampening=0.1), ValueError, "nesterov"),
           (dict(type="SGD", momentum=-0.1), ValueError, "momentum"), (dict(type="Adam", betas=[0.9, 1.0]), ValueError, "betas"),
           (dict(type="Adam", betas=[0.9]), ValueError, "betas"), (dict(type="AdamW", eps=-1e-8), ValueError, "eps"),
           (dict(type="RMSprop", alpha=-0.5), ValueError, "alpha"), (dict(type="Adam", weight_decay=-0.1), ValueError, "weight_decay"),
           (dict(type="Adam", lr=-1e-4), ValueError, "lr"), (dict(type="Adam", amsgrad="yes"), ValueError, "amsgrad")]


@pytest.mark.parametrize("block,exc,word", REFUSED, ids=[f"{b['type']}-{w}" for b, _, w in REFUSED])
def test_each_refusal_names_its_key_or_type(block, exc, word):
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    block = dict({"lr": 1e-4}, **block)
    for name in ("optim_g", "optim_d"):
        with pytest.raises(exc, match=rf"train\.{name}.*{word}"):
            train_config_from_opt(_with(_shipped(), name, block))
    if exc is ValueError and block["type"] in ("SGD", "Adam", "AdamW", "RMSprop") and word not in ("amsgrad",) and block.get("betas") != [0.9]:
        with pytest.raises(ValueError):                 # "the way torch does"
            getattr(torch.optim, block["type"])([torch.nn.Parameter(torch.zeros(2))], **{k: v for k, v in block.items() if k != "type"})


def test_step_config_from_opt_still_refuses_the_same_options():
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt
    for path, val, key in ((("optim_g", "type"), "AdamW", r"optim_g\.type"), (("optim_d", "type"), "RMSprop", r"optim_d\.type"),
                           (("optim_d", "weight_decay"), 0.1, "weight_decay"), (("optim_g", "amsgrad"), True, "amsgrad"),
                           (("scheduler", "type"), "CosineAnnealingRestartLR", r"scheduler\.type"),
                           (("scheduler", "restarts"), [0, 100], "restarts"), (("scheduler", "restart_weights"), [0.5], "restarts")):
        o = _shipped()
        o["train"][path[0]][path[1]] = val
        with pytest.raises(NotImplementedError, match=key):
            step_config_from_opt(o)


def test_scheduler_options_parse_or_are_refused_by_name():
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    o = _shipped()
    o["train"]["total_iter"] = 400
    o["train"]["scheduler"] = {"type": "CosineAnnealingRestartLR", "periods": [100, 300], "restart_weights": [1, 0.5], "eta_min": 1e-7}
    assert train_config_from_opt(o).lr_g == 1e-4
    o["train"]["total_iter"] = 500                       # the schedule ends before the training does: refused at construction
    with pytest.raises(ValueError, match="periods"):
        train_config_from_opt(o)
    o["train"]["scheduler"] = {"type": "MultiStepRestartLR", "milestones": [10, 20], "gamma": 0.5, "restarts": [0, 15], "restart_weights": [1, 0.5]}
    train_config_from_opt(o)
    with pytest.raises(ValueError, match="restart_weights"):
        O.Schedule({"type": "MultiStepRestartLR", "milestones": [1], "restarts": [0, 5], "restart_weights": [1]})
    with pytest.raises(NotImplementedError, match="CosineAnnealingLR"):
        O.Schedule({"type": "CosineAnnealingLR", "T_max": 10})
    with pytest.raises(NotImplementedError, match="T_max"):
        O.Schedule({"type": "MultiStepLR", "milestones": [1], "T_max": 10})
    s = O.Schedule({"type": "CosineAnnealingRestartLR", "periods": [4], "restart_weights": [1]})       # total_iter unknown:
    s.lr(1e-4, 5)                                                                                  # last_epoch 4 = the period's end
    with pytest.raises(IndexError, match="past the last period"):                                  # raised when reached, never continued
        s.lr(1e-4, 6)


# ================================================================================================ schedules
def _chained_multistep(base, n, milestones, gamma, restarts, weights):
    """[recalled] basicsr MultiStepRestartLR stepped epoch by epoch: get_lr() at last_epoch = 0 on construction, then once per step()"""
    from collections import Counter
    ms = Counter(milestones)
    lr, out = base, []
    for e in range(n):
        if e in restarts:
            lr = base * weights[restarts.index(e)]           # initial_lr * weight: wins over a milestone at the same epoch
        elif e in ms:
            lr = lr * gamma ** ms[e]
        out.append(lr)
    return out


# Bit equality, not 1 ulp.  Why it can be asked: in the first four schedules gamma and every weight are powers of two, so every product
# of the chain and of the closed form is exact.  In the last two (gamma 0.1, weights 1) at most one milestone EPOCH lies in a
# segment, so the chain does base * gamma**c once - the very operation of the closed form (1.0 * x is exact).
MULTISTEP = [
    dict(milestones=[5, 9, 14], gamma=0.5, restarts=[0], weights=[1]),                               # no restart
    dict(milestones=[3, 3, 8, 12, 12, 12], gamma=0.5, restarts=[0], weights=[1]),                    # repeated milestones
    dict(milestones=[4, 12, 15], gamma=0.25, restarts=[0, 10], weights=[1, 0.5]),                    # a restart
    dict(milestones=[4, 10, 10, 13], gamma=0.5, restarts=[0, 10, 16], weights=[1, 0.5, 0.25]),       # a restart ON a (repeated) milestone
    dict(milestones=[7, 7], gamma=0.1, restarts=[0], weights=[1]),                                   # non-dyadic gamma, a repeated milestone
    dict(milestones=[4, 13], gamma=0.1, restarts=[0, 10], weights=[1, 1]),
]


@pytest.mark.parametrize("sc", MULTISTEP, ids=[str(i) for i in range(len(MULTISTEP))])
def test_multistep_closed_form_equals_the_chained_scheduler_bit_for_bit(sc):
    from satlas_super_resolution_amd import optimizers as O
    base, n = 1e-4, 20
    chain = _chained_multistep(base, n, sc["milestones"], sc["gamma"], sc["restarts"], sc["weights"])
    sched = O.Schedule({"type": "MultiStepRestartLR", "milestones": sc["milestones"], "gamma": sc["gamma"], "restarts": sc["restarts"],
                        "restart_weights": sc["weights"]})
    for e in range(n):
        got = O.multistep_restart_lr(base, e, sc["milestones"], sc["gamma"], sc["restarts"], sc["weights"])
        assert got == chain[e], (e, got, chain[e])                       # equal to the last bit of a double
        assert sched.lr(base, e + 1) == got                              # last_epoch = current_iter - 1
    if sc["restarts"] == [0] and sc["weights"] == [1]:                  # no restarts: torch's own MultiStepLR, stepped
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=base)
        ts = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=sc["milestones"], gamma=sc["gamma"])
        for e in range(n):
            assert opt.param_groups[0]["lr"] == chain[e], (e, opt.param_groups[0]["lr"], chain[e])
            opt.step()
            ts.step()


def test_warmup_stays_base_times_iter_over_warmup():
    from satlas_super_resolution_amd import optimizers as O
    s = O.Schedule({"type": "MultiStepLR", "milestones": [3], "gamma": 0.5})
    assert s.lr(2e-4, 1, 10) == 2e-4 * (1 / 10) and s.lr(2e-4, 9, 10) == 2e-4 * (9 / 10)
    assert s.lr(2e-4, 10, 10) == 1e-4 and s.lr(2e-4, 3, -1) == 2e-4 and s.lr(2e-4, 4, -1) == 1e-4
    assert O.Schedule(None).lr(3e-4, 1000) == 3e-4


def _stepped_cosine(base, periods, weights, eta_min):
    """[recalled] basicsr CosineAnnealingRestartLR, one get_lr() per epoch from last_epoch = 0, restated from its source: cumulative
    periods, get_position_from_periods (first index whose cumulative period is >= the epoch)"""
    cum = [sum(periods[:i + 1]) for i in range(len(periods))]
    out = []
    for e in range(cum[-1] + 1):
        idx = next(i for i, c in enumerate(cum) if e <= c)
        nearest = 0 if idx == 0 else cum[idx - 1]
        out.append(eta_min + weights[idx] * 0.5 * (base - eta_min) * (1 + math.cos(math.pi * ((e - nearest) / periods[idx]))))
    return cum, out


@pytest.mark.parametrize("periods,weights,eta_min", [([10, 10], [1, 1], 0.0), ([7, 13, 5], [1, 0.5, 0.3], 1e-7), ([1, 4], [1, 0.7], 1e-6)])
def test_cosine_restart_closed_form(periods, weights, eta_min):
    """Equal to the last bit of a double: BasicSR's get_lr is itself a closed form in last_epoch, and the implementation evaluates the
    same expression in the same order.  The first and the last iteration of every period are checked against their exact values."""
    from satlas_super_resolution_amd import optimizers as O
    base = 2e-4
    cum, ref = _stepped_cosine(base, periods, weights, eta_min)
    sched = O.Schedule({"type": "CosineAnnealingRestartLR", "periods": periods, "restart_weights": weights, "eta_min": eta_min})
    for e, r in enumerate(ref):
        assert O.cosine_restart_lr(base, e, periods, weights, eta_min) == r, (e, r)
        assert sched.lr(base, e + 1) == r
    for idx, p in enumerate(periods):
        start = 0 if idx == 0 else cum[idx - 1]
        first = start if idx == 0 else start + 1            # epoch `start` itself is the END of the period before
        peak = eta_min + weights[idx] * 0.5 * (base - eta_min) * (1 + math.cos(math.pi * ((first - start) / p)))
        assert O.cosine_restart_lr(base, first, periods, weights, eta_min) == peak
        if idx == 0:
            assert peak == eta_min + weights[0] * 0.5 * (base - eta_min) * 2.0      # cos(0) = 1: the full base LR (weight 1)
        assert O.cosine_restart_lr(base, cum[idx], periods, weights, eta_min) == eta_min      # 1 + cos(pi) = 0 exactly
    with pytest.raises(IndexError):
        O.cosine_restart_lr(base, cum[-1] + 1, periods, weights, eta_min)


def test_scheduler_state_dicts_have_the_schedulers_attributes():
    from collections import Counter
    from satlas_super_resolution_amd import optimizers as O
    m = O.Schedule({"type": "MultiStepRestartLR", "milestones": [3, 3, 9], "gamma": 0.5, "restarts": [0, 5], "restart_weights": [1, 0.5]})
    sd = m.state_dict(1e-4, 2.5e-5, 5)
    assert sd == {"milestones": Counter({3: 2, 9: 1}), "gamma": 0.5, "restarts": [0, 5], "restart_weights": [1.0, 0.5], "base_lrs": [1e-4],
                  "last_epoch": 4, "_step_count": 5, "verbose": False, "_get_lr_called_within_step": False, "_last_lr": [2.5e-5]}
    c = O.Schedule({"type": "CosineAnnealingRestartLR", "periods": [10, 20], "restart_weights": [1, 0.5], "eta_min": 1e-7})
    sd = c.state_dict(1e-4, 5e-5, 6)
    assert sd["periods"] == [10, 20] and sd["cumulative_period"] == [10, 30] and sd["eta_min"] == 1e-7 and sd["restart_weights"] == [1.0, 0.5]
    assert sd["last_epoch"] == 5 and sd["base_lrs"] == [1e-4] and sd["_last_lr"] == [5e-5]
    assert "optimizer" not in sd


# ================================================================================================ checkpoint layout
KINDS = [dict(type="Adam", lr=1e-3, weight_decay=0.01), dict(type="Adam", lr=1e-3, amsgrad=True), dict(type="AdamW", lr=1e-3, amsgrad=True),
         dict(type="AdamW", lr=1e-3), dict(type="SGD", lr=1e-2), dict(type="SGD", lr=1e-2, momentum=0.9, nesterov=True),
         dict(type="RMSprop", lr=1e-3), dict(type="RMSprop", lr=1e-3, momentum=0.5), dict(type="RMSprop", lr=1e-3, centered=True),
         dict(type="RMSprop", lr=1e-3, momentum=0.5, centered=True)]
SHAPES = [(4, 3, 3, 3), (4,), (2, 4, 1, 1)]


def _ident(b):
    return "-".join([b["type"]] + [k for k in ("weight_decay", "amsgrad", "momentum", "nesterov", "centered") if b.get(k)])


@pytest.mark.parametrize("block", KINDS, ids=[_ident(b) for b in KINDS])
def test_saved_state_dict_is_what_torch_optim_writes_and_loads(block):
    """optimizers.optimizer_state_dict - the save path - from CPU tensors: the same keys, key for key, as the state_dict() of the
    installed torch.optim class after two steps on same-shaped parameters; load_state_dict accepts it; it round-trips."""
    from satlas_super_resolution_amd import optimizers as O
    spec = O.normalize_optim("optim_g", block)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s)) for s in SHAPES]
    kw = {k: v for k, v in spec.items() if k != "type"}
    ref = getattr(torch.optim, spec["type"])(params, **kw)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn_like(p)
        ref.step()
    want = ref.state_dict()
    # the arenas the device would hold: one flat tensor per state key, sliced per parameter
    per = [{k: torch.randn(s) for k in O.state_keys(spec)} for s in SHAPES]
    got = O.optimizer_state_dict(spec, 5e-4, per, step=2)
    assert set(got) == set(want) == {"state", "param_groups"}
    gg, wg = got["param_groups"][0], want["param_groups"][0]
    assert list(gg) == list(wg) + ["initial_lr"]            # BasicSR's scheduler adds initial_lr to the group
    for k in wg:
        if k != "lr":
            assert gg[k] == wg[k] and type(gg[k]) is type(wg[k]), k
    assert gg["lr"] == 5e-4 and gg["initial_lr"] == spec["lr"]
    assert list(got["state"]) == list(want["state"])
    for i in want["state"]:
        assert list(got["state"][i]) == list(want["state"][i]), (i, list(got["state"][i]), list(want["state"][i]))
        for k, v in want["state"][i].items():
            g = got["state"][i][k]
            assert g.shape == v.shape and g.dtype == v.dtype, (i, k)
            if k == "step":
                assert float(g) == float(v) == 2.0
            else:
                assert torch.equal(g, per[i][k])
    fresh = getattr(torch.optim, spec["type"])([torch.nn.Parameter(torch.zeros(s)) for s in SHAPES], **kw)
    fresh.load_state_dict(got)
    back = fresh.state_dict()
    assert back["param_groups"] == got["param_groups"]
    for i in got["state"]:
        assert list(back["state"][i]) == list(got["state"][i])
        for k, v in got["state"][i].items():
            assert torch.equal(back["state"][i][k], v), (i, k)
    # the resume side reads back what the save side wrote
    assert O.state_dict_type(got) == spec["type"]
    O.check_resume_type("optim_g", spec, got)
    assert O.resumed_step(spec, got) == (2 if spec["type"] != "SGD" else (1 if spec["momentum"] else 0))
    # before the first applied step torch holds no state
    assert O.optimizer_state_dict(spec, 5e-4, per, step=0)["state"] == {}


def test_state_of_another_optimizer_type_is_refused_by_name():
    from satlas_super_resolution_amd import optimizers as O
    specs = {b["type"]: O.normalize_optim("optim_d", b) for b in (KINDS[0], KINDS[3], KINDS[5], KINDS[7])}
    sds = {t: O.optimizer_state_dict(s, 1e-3, [{k: torch.zeros(3) for k in O.state_keys(s)}], step=1) for t, s in specs.items()}
    for mine, spec in specs.items():
        for wrote, sd in sds.items():
            if wrote == mine:
                O.check_resume_type("optim_d", spec, sd)
            else:
                with pytest.raises(ValueError, match=rf"optim_d.*{wrote}.*{mine}"):
                    O.check_resume_type("optim_d", spec, sd)
    ams = O.normalize_optim("optim_d", dict(type="Adam", lr=1e-3, weight_decay=0.01, amsgrad=True))
    with pytest.raises(ValueError, match="max_exp_avg_sq"):          # same type, but the state lacks an arena the options need
        O.check_resume_type("optim_d", ams, sds["Adam"])
