"""GPU: ssr_optim_step / ssr_optim_step_guarded (csrc/optim.hip) - Adam with weight decay / amsgrad, AdamW, SGD, RMSprop + the fused EMA -
through the C ABI, through the whole train step and through the model plugin, each held to the single-tensor arithmetic of the
installed torch.optim restated in float64.

Bounds.  The float64 restatement carries, next to every value, a first-order bound on what fp32 arithmetic can be away from it (class
E): an operation's result inherits its operands' bounds through the operation's derivatives and adds one rounding, U |result|
(U = 2^-24; conventions of tests/test_gpu_support_kernels.py, whose helpers are imported).  A hyper-parameter the kernel holds as an
fp32 constant is off by at most U |c|; 1 - beta^t is off by bias_correction_term (powf on the fp32-rounded beta).  A fused multiply-add
only removes a rounding.  Criterion everywhere: error / bound <= 1, element by element.

Centered RMSprop takes sqrt(square_avg - grad_avg^2) and, like torch, does not clamp: the state of the single-launch cases is built
with square_avg >= 4 grad_avg^2, so that the float64 radicand stays well away from 0, where an fp32 radicand may go negative."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_support_kernels import (ADAM_CAP, ADAM_PER_BLOCK, U, _adam_state, _fresh_grad, bias_correction_term, guarded_from, past_cap,
                                      same_bits, within)

pytestmark = pytest.mark.gpu

DECAY = 0.999


# ================================================================================================ float64 + error bound
class E:
    """a float64 value and a bound on |fp32 evaluation - value|, propagated to first order with one rounding per operation"""

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.v = self.v.double()
        self.e = torch.zeros_like(self.v) if e is None else (e if torch.is_tensor(e) else torch.tensor(float(e), dtype=torch.float64))

    @staticmethod
    def const(c):
        """a Python-double hyper-parameter the kernel holds rounded to fp32"""
        return E(c, U * abs(c))

    def _r(self, v, e):
        return E(v, e + U * (v.abs() + e))          # the rounding is relative to the fp32 operands' result: at most |v| + e

    def __add__(self, o):
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return self._r(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)

    def __truediv__(self, o):
        q = self.v / o.v
        return self._r(q, self.e / o.v.abs() + q.abs() * o.e / (o.v.abs() - o.e).clamp_min(1e-300))

    def sqrt(self):
        s = self.v.sqrt()
        return self._r(s, self.e / (s + (self.v - self.e).clamp_min(0).sqrt()).clamp_min(1e-300))

    def maximum(self, o):
        return E(torch.maximum(self.v, o.v), torch.maximum(self.e, o.e))      # a selection: no rounding


ONE = E(1.0)


def _one_minus_pow(beta, t):
    v = 1.0 - beta ** t
    return E(v, bias_correction_term(beta, t) * v)


def reference(spec, st, lr32, t0, scale, decay, with_ema):
    """One step of torch.optim.<spec type> (single-tensor path: adam.py _single_tensor_adam, sgd.py _single_tensor_sgd, rmsprop.py
    _single_tensor_rmsprop of the installed torch) in float64 on the state `st` (float64 tensors by torch state key, + param, grad, ema),
    followed by BasicSR's model_ema; `t0` applied steps so far.  Returns {name: E} for the parameter, the EMA and every state arena."""
    typ = spec["type"]
    lr = E(lr32)
    g = E(st["grad"]) * E(scale)
    p = E(st["param"])
    wd = spec["weight_decay"]
    out = {}
    if typ in ("Adam", "AdamW"):
        b1, b2 = spec["betas"]
        t = t0 + 1
        if wd != 0:
            if typ == "AdamW":
                p = p * (ONE - lr * E.const(wd))                                  # param.mul_(1 - lr * weight_decay)
            else:
                g = g + E.const(wd) * p                                           # grad.add(param, alpha=weight_decay)
        m, v = E(st["exp_avg"]), E(st["exp_avg_sq"])
        m = m + (g - m) * (ONE - E.const(b1))                                     # exp_avg.lerp_(grad, 1 - beta1)
        v = v * E.const(b2) + (ONE - E.const(b2)) * g * g                         # mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        out["exp_avg"], out["exp_avg_sq"] = m, v
        vd = v
        if spec["amsgrad"]:
            vd = E(st["max_exp_avg_sq"]).maximum(v)                               # torch.maximum(max_exp_avg_sqs[i], exp_avg_sq, out=...)
            out["max_exp_avg_sq"] = vd
        step_size = lr / _one_minus_pow(b1, t)
        denom = vd.sqrt() / _one_minus_pow(b2, t).sqrt() + E.const(spec["eps"])
        p = p - step_size * (m / denom)                                           # param.addcdiv_(exp_avg, denom, value=-step_size)
    elif typ == "SGD":
        mom = spec["momentum"]
        if wd != 0:
            g = g + E.const(wd) * p
        if mom != 0:
            if t0 == 0:
                buf = g                                                           # buf = grad.clone(): the buffer does not exist yet
            else:
                buf = E(st["momentum_buffer"]) * E.const(mom) + (ONE - E.const(spec["dampening"])) * g
            out["momentum_buffer"] = buf
            g = g + E.const(mom) * buf if spec["nesterov"] else buf
        p = p - lr * g
    else:
        alpha, mom = spec["alpha"], spec["momentum"]
        if wd != 0:
            g = g + E.const(wd) * p
        sq = E(st["square_avg"]) * E.const(alpha) + (ONE - E.const(alpha)) * g * g
        out["square_avg"] = sq
        if spec["centered"]:
            ga = E(st["grad_avg"])
            ga = ga + (g - ga) * (ONE - E.const(alpha))                           # grad_avg.lerp_(grad, 1 - alpha)
            out["grad_avg"] = ga
            avg = (sq - ga * ga).sqrt()                                           # square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
        else:
            avg = sq.sqrt()
        avg = avg + E.const(spec["eps"])
        if mom > 0:
            buf = E(st["momentum_buffer"]) * E.const(mom) + g / avg               # buf.mul_(momentum).addcdiv_(grad, avg)
            out["momentum_buffer"] = buf
            p = p - lr * buf
        else:
            p = p - lr * (g / avg)
    out["param"] = p
    if with_ema:
        out["ema"] = E(st["ema"]) * E.const(decay) + p * (ONE - E.const(decay))
    return out


def torch_optim_step(spec, st, lr32, t0, scale):
    """the same step by the installed torch.optim class itself, on float64 CPU tensors (the definition the restatement is held to)"""
    from satlas_super_resolution_amd import optimizers as O
    p = torch.nn.Parameter(st["param"].double().clone())
    kw = {k: v for k, v in spec.items() if k not in ("type", "lr")}
    opt = getattr(torch.optim, spec["type"])([p], lr=lr32, foreach=False, **kw)
    keys = O.state_keys(spec)
    if t0 > 0:
        state = {k: st[k].double().clone() for k in keys}
        if O.has_step(spec):
            state["step"] = torch.tensor(float(t0), dtype=torch.float64)
        if state:
            opt.load_state_dict({"state": {0: state}, "param_groups": opt.state_dict()["param_groups"]})
    p.grad = st["grad"].double() * scale
    opt.step()
    out = {"param": p.detach()}
    for k in keys:
        out[k] = opt.state[p][k]
    return out


# ================================================================================================ cases
from satlas_super_resolution_amd.optimizers import normalize_optim, state_keys   # noqa: E402  (host-only imports)

WD = 0.01
BLOCKS = [dict(type="Adam"), dict(type="Adam", weight_decay=WD), dict(type="Adam", amsgrad=True), dict(type="Adam", weight_decay=WD, amsgrad=True),
          dict(type="AdamW", weight_decay=WD), dict(type="AdamW", weight_decay=WD, amsgrad=True), dict(type="AdamW", weight_decay=0.0),
          dict(type="SGD"), dict(type="SGD", weight_decay=WD), dict(type="SGD", momentum=0.9), dict(type="SGD", momentum=0.9, dampening=0.1, weight_decay=WD),
          dict(type="SGD", momentum=0.9, nesterov=True), dict(type="SGD", momentum=0.9, nesterov=True, weight_decay=WD)] + \
         [dict(type="RMSprop", alpha=0.99 if c else 0.9, momentum=m, centered=c, weight_decay=w) for m in (0.0, 0.5) for c in (False, True) for w in (0.0, WD)]
LR = {"Adam": 1e-4, "AdamW": 1e-4, "SGD": 1e-2, "RMSprop": 1e-4}


def _spec(block, betas=(0.9, 0.99)):
    b = dict(block, lr=LR[block["type"]])
    if b["type"] in ("Adam", "AdamW"):
        b["betas"] = betas
    return normalize_optim("optim", b)


def _ident(block):
    return "-".join([block["type"]] + [f"{k}{block[k] if not isinstance(block[k], bool) else ''}" for k in sorted(block) if k != "type" and block[k]])


PAST = past_cap(ADAM_PER_BLOCK, ADAM_CAP)                  # csrc/optim.hip sizes its grid like ssr_adam_step: grid_for(n, 256 * 4, 2048)
# (n, with_ema, grad_scale, step counter): every size, both EMA settings, both scales and all three counters for every option combination
LAUNCHES = [(100003, True, 0.125, 0), (100003, False, 1.0, 1), (100003, True, 1.0, 999), (1, True, 1.0, 0), (1, False, 0.125, 999),
            (PAST, True, 0.125, 1)]


def _state(spec, n, seed, moments=True):
    """state built like _adam_state (magnitudes over eight decades, exact zeros, every 97th element all-zero) under torch's state keys"""
    s = _adam_state(n, seed, moments)
    st = {"param": s["param"], "grad": s["grad"], "ema": s["ema"]}
    flip = torch.where(torch.arange(n) % 2 == 0, 0.5, 2.0)
    # centered RMSprop: |grad_avg| <= sqrt(square_avg) / 2, i.e. square_avg >= 4 grad_avg^2 (module docstring)
    full = {"exp_avg": s["m"], "exp_avg_sq": s["v"], "max_exp_avg_sq": s["v"] * flip,       # the running max is above / below exp_avg_sq in turn
            "momentum_buffer": s["m"], "square_avg": s["v"], "grad_avg": s["m"].sign() * torch.minimum(s["m"].abs(), 0.5 * s["v"].sqrt())}
    for k in state_keys(spec):
        st[k] = full[k].float()
        if k == "grad_avg":
            assert bool((st["square_avg"].double() >= 4 * st["grad_avg"].double() ** 2 * (1 - 1e-6)).all())
    return st


def _args(spec, dev, lr, step, scale, decay, with_ema):
    from satlas_super_resolution_amd import optimizers as O
    ptrs = {k: g.ptr() for k, g in dev.items() if k != "ema"}
    ptrs.update(lr=lr.ptr(), step=step.data_ptr(), ema=dev["ema"].ptr() if with_ema else None)
    return O.optim_args(spec, ptrs, dev["param"].n, decay, scale)


def _launch(spec, dev, lr, step, scale, decay, with_ema, guard=None):
    from satlas_super_resolution_amd import hip
    a = _args(spec, dev, lr, step, scale, decay, with_ema)
    if guard is None:
        hip.check(hip.lib().ssr_optim_step(C.byref(a), hip.stream_ptr()), "ssr_optim_step")
    else:
        flag, skipped = guard
        hip.check(hip.lib().ssr_optim_step_guarded(C.byref(a), flag.data_ptr(), skipped.data_ptr(), hip.stream_ptr()), "ssr_optim_step_guarded")


def _check(tag, spec, dev, before, lr32, t0, scale, decay, with_ema):
    ref = reference(spec, {k: x.double() for k, x in before.items()}, lr32, t0, scale, decay, with_ema)
    got = {k: dev[k].t.cpu() for k in dev}
    worst = {}
    for k, r in ref.items():
        worst[k] = within(got[k], r.v, r.e)[1]
    if not with_ema:
        assert same_bits(got["ema"], before["ema"])              # ema = NULL: the arena stays as it is
    assert same_bits(got["grad"], before["grad"])
    if spec["weight_decay"] == 0:
        # all-zero state and gradient: an update of exactly 0 (with weight decay the update is -lr wd p by definition)
        dead = before["grad"] == 0
        for k in state_keys(spec):
            dead &= before[k] == 0
        assert int(dead.sum()) >= 1 or dev["param"].n < 97
        assert same_bits(got["param"][dead], before["param"][dead])
        for k in state_keys(spec):
            assert bool((got[k][dead] == 0).all()), k
    assert all(x.margins_intact() for x in dev.values())
    line = f"optim_step {tag}: " + " ".join(f"{k} {r:.3f}" for k, r in worst.items()) + "  (error / bound, bound 1)"
    print(line)
    for k, r in worst.items():
        assert r <= 1.0, (tag, k, r)


@pytest.mark.parametrize("launch", LAUNCHES, ids=[f"n{n}-{'ema' if e else 'noema'}-scale{s}-step{t}" for n, e, s, t in LAUNCHES])
@pytest.mark.parametrize("block", BLOCKS, ids=[_ident(b) for b in BLOCKS])
def test_single_launch_against_float64(block, launch):
    n, with_ema, scale, step0 = launch
    spec = _spec(block, betas=(0.9, 0.999) if step0 == 999 else (0.9, 0.99))
    before = _state(spec, n, seed=step0 + n)
    dev = {k: guarded_from(x) for k, x in before.items()}
    glr = guarded_from(torch.tensor([spec["lr"]]))
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    _launch(spec, dev, glr, step, scale, DECAY, with_ema)
    assert int(step.item()) == step0 + 1
    _check(f"{_ident(block)} t0={step0} n={n}", spec, dev, before, float(np.float32(spec["lr"])), step0, scale, DECAY, with_ema)


@pytest.mark.parametrize("block", BLOCKS, ids=[_ident(b) for b in BLOCKS])
def test_three_consecutive_launches_from_empty_state(block):
    """from zero arenas and step 0; SGD with dampening: the first applied step sets momentum_buffer = g, not (1 - dampening) g.  The
    float64 restatement is itself held to the installed torch.optim class, stepped in float64 from the same state."""
    n, scale = 100003, 0.5
    spec = _spec(block)
    before = _state(spec, n, seed=4, moments=False)
    dev = {k: guarded_from(x) for k, x in before.items()}
    glr = guarded_from(torch.tensor([spec["lr"]]))
    lr32 = float(np.float32(spec["lr"]))
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t0 in (0, 1, 2):
        if t0 > 0:
            dev["grad"].t.copy_(_fresh_grad(n, 40 + t0))
        before = {k: x.t.cpu().clone() for k, x in dev.items()}
        _launch(spec, dev, glr, step, scale, DECAY, True)
        _check(f"{_ident(block)} consecutive t0={t0}", spec, dev, before, lr32, t0, scale, DECAY, True)
        ref = reference(spec, {k: x.double() for k, x in before.items()}, lr32, t0, scale, DECAY, False)
        tor = torch_optim_step(spec, before, lr32, t0, scale)
        for k, v in tor.items():          # two float64 evaluations of one formula: 1e-12 relative is far below any fp32 bound
            assert float((v - ref[k].v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), (k, t0)
    assert int(step.item()) == 3


@pytest.mark.parametrize("n", [1, 100003, PAST])
def test_plain_adam_through_the_new_entry_points_is_ssr_adam_step_bit_for_bit(n):
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    spec = _spec(dict(type="Adam"))
    before = _state(spec, n, seed=11)
    lr = guarded_from(torch.tensor([1e-4]))
    runs = []
    for which in ("adam", "optim", "adam_guarded", "optim_guarded"):
        dev = {k: guarded_from(x) for k, x in before.items()}
        step = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        flag, skipped = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        if which.startswith("adam"):
            a = hip.AdamArgs(dev["param"].ptr(), dev["grad"].ptr(), dev["exp_avg"].ptr(), dev["exp_avg_sq"].ptr(), dev["ema"].ptr(), n, lr.ptr(),
                             step.data_ptr(), 0.9, 0.99, 1e-8, DECAY, 0.125)
            if which == "adam":
                hip.check(L.ssr_adam_step(C.byref(a), hip.stream_ptr()), which)
            else:
                hip.check(L.ssr_adam_step_guarded(C.byref(a), flag.data_ptr(), skipped.data_ptr(), hip.stream_ptr()), which)
        else:
            _launch(spec, dev, lr, step, 0.125, DECAY, True, guard=(flag, skipped) if which == "optim_guarded" else None)
        assert int(step.item()) == 8 and int(skipped.item()) == 0
        runs.append({k: x.t.cpu() for k, x in dev.items()})
    for other in runs[1:]:
        for k in runs[0]:
            assert same_bits(other[k], runs[0][k]), k
    assert not same_bits(runs[0]["param"], before["param"]) or n == 1


@pytest.mark.parametrize("block", BLOCKS, ids=[_ident(b) for b in BLOCKS])
def test_guarded_launch(block):
    """flagged: every arena and `step` bit-identical, only the EMA moves (toward the unchanged parameters), the skip is counted, the
    flag cleared.  Unflagged: the plain launch bit for bit."""
    n, step0, scale = 4099, 1, 0.125
    spec = _spec(block)
    before = _state(spec, n, seed=21)
    lr = guarded_from(torch.tensor([spec["lr"]]))
    # ---- flagged
    dev = {k: guarded_from(x) for k, x in before.items()}
    step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
    flag, skipped = torch.ones(1, dtype=torch.int32, device="cuda"), torch.full((1,), 5, dtype=torch.int32, device="cuda")
    _launch(spec, dev, lr, step, scale, DECAY, True, guard=(flag, skipped))
    assert (int(step.item()), int(flag.item()), int(skipped.item())) == (step0, 0, 6)
    for k in dev:
        if k != "ema":
            assert same_bits(dev[k].t, before[k]), k
    ema = E(before["ema"].double()) * E.const(DECAY) + E(before["param"].double()) * (ONE - E.const(DECAY))
    assert within(dev["ema"].t.cpu(), ema.v, ema.e)[1] <= 1.0
    assert not same_bits(dev["ema"].t, before["ema"])
    assert all(x.margins_intact() for x in dev.values())
    # ---- flagged, no EMA: nothing moves at all
    dev = {k: guarded_from(x) for k, x in before.items()}
    flag.fill_(1)
    _launch(spec, dev, lr, step, scale, DECAY, False, guard=(flag, skipped))
    assert (int(step.item()), int(flag.item()), int(skipped.item())) == (step0, 0, 7)
    assert all(same_bits(dev[k].t, before[k]) for k in dev)
    # ---- unflagged guarded == plain
    runs = []
    for guarded in (False, True):
        dev = {k: guarded_from(x) for k, x in before.items()}
        step = torch.full((1,), step0, dtype=torch.int32, device="cuda")
        _launch(spec, dev, lr, step, scale, DECAY, True, guard=(flag, skipped) if guarded else None)
        assert int(step.item()) == step0 + 1 and int(flag.item()) == 0 and int(skipped.item()) == 7
        runs.append({k: x.t.cpu() for k, x in dev.items()})
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), k
    assert not same_bits(runs[0]["param"], before["param"])


def test_bad_arguments_are_refused_without_a_launch():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    n = 8
    t = {k: torch.zeros(n, device="cuda") for k in ("param", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer", "square_avg", "grad_avg")}
    lr, step = torch.ones(1, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")

    def rc(spec, drop=(), **over):
        from satlas_super_resolution_amd import optimizers as O
        ptrs = {k: (None if k in drop else v.data_ptr()) for k, v in t.items()}
        ptrs.update(lr=lr.data_ptr(), step=step.data_ptr(), ema=None)
        a = O.optim_args(spec, ptrs, n)
        for k, v in over.items():
            setattr(a, k, v)
        return L.ssr_optim_step(C.byref(a), hip.stream_ptr())
    assert rc(_spec(dict(type="Adam", amsgrad=True)), drop=("max_exp_avg_sq",)) == -1
    assert rc(_spec(dict(type="AdamW", weight_decay=WD)), drop=("exp_avg_sq",)) == -1
    assert rc(_spec(dict(type="SGD", momentum=0.9)), drop=("momentum_buffer",)) == -1
    assert rc(_spec(dict(type="SGD", momentum=0.9)), flags=hip.OPT_NESTEROV, dampening=0.1) == -1
    assert rc(_spec(dict(type="SGD")), flags=hip.OPT_NESTEROV) == -1
    assert rc(_spec(dict(type="RMSprop", centered=True)), drop=("grad_avg",)) == -1
    assert rc(_spec(dict(type="RMSprop", momentum=0.5)), drop=("momentum_buffer",)) == -1
    assert rc(_spec(dict(type="RMSprop")), kind=9) == -2
    assert rc(_spec(dict(type="RMSprop")), n=0) == -1
    torch.cuda.synchronize()
    assert int(step.item()) == 0 and all(float(v.abs().sum()) == 0 for v in t.values())


# ================================================================================================ the whole step
def _tiny():
    from test_gpu_boundary import _tiny as tiny
    return tiny()


def _snapshot(o, store):
    s = {"param": store.data, "ema": o.ema if o.ema is not None else store.data}
    s.update(o.arenas)
    return {k: v.detach().cpu().clone() for k, v in s.items()}


STEP_CASES = {
    "adamw_amsgrad+rmsprop_momentum": (dict(type="AdamW", lr=1e-3, betas=(0.9, 0.99), weight_decay=0.01, amsgrad=True),
                                       dict(type="RMSprop", lr=1e-4, momentum=0.5)),
    "sgd_nesterov": (dict(type="SGD", lr=1e-2, momentum=0.9, nesterov=True), dict(type="SGD", lr=1e-2, momentum=0.9, nesterov=True)),
}


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_whole_step_follows_torch_optim(case, use_graph):
    """B = 2, 8 x 8 input, exact fp32, three iterations (with graphs: first touch, capture, replay).  After each iteration the gradient
    arenas are read back and the installed torch.optim class steps float64 copies of the previous parameters and state from them on the
    CPU: parameters, EMA and every state arena of the device stay within the single-launch bounds of that step."""
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw, d_kw, g0, d0 = _tiny()
    bg, bd = STEP_CASES[case]
    sg, sd = O.normalize_optim("optim_g", bg), O.normalize_optim("optim_d", bd)
    cfg = StepConfig(ema_decay=0.9, lr_g=sg["lr"], lr_d=sd["lr"], optim_g=sg, optim_d=sd)
    ts = ESRGANTrainStep(g_kw, d_kw, 2, 8, 8, "fp32", cfg, use_graph=use_graph)
    ts.load_state(g0, d0)
    assert type(ts.opt_g) is O.OptimState and type(ts.opt_d) is O.OptimState
    assert list(ts.opt_g.arenas) == O.state_keys(sg) and list(ts.opt_d.arenas) == O.state_keys(sd)
    torch.manual_seed(5)
    data = [(torch.rand(2, 6, 8, 8), torch.rand(2, 3, 32, 32)) for _ in range(3)]
    for it, (lr, gt) in enumerate(data, start=1):
        before = [_snapshot(o, st) for o, st in ((ts.opt_g, ts.g_store), (ts.opt_d, ts.d_store))]
        ts.feed_data(lr.cuda(), gt.cuda())
        ts.step(it)
        torch.cuda.synchronize()
        for name, o, st, spec, b, decay in (("G", ts.opt_g, ts.g_store, sg, before[0], 0.9), ("D", ts.opt_d, ts.d_store, sd, before[1], 0.0)):
            assert int(o.step.item()) == it and int(o.skipped.item()) == 0
            b["grad"] = st.grad.detach().cpu().clone()
            assert bool(torch.isfinite(b["grad"]).all()) and float(b["grad"].abs().max()) > 0
            lr32 = float(o.lr.item())
            ref = reference(spec, {k: x.double() for k, x in b.items()}, lr32, it - 1, 1.0, decay, decay > 0)
            tor = torch_optim_step(spec, b, lr32, it - 1, 1.0)
            after = _snapshot(o, st)
            for k, r in ref.items():
                if k in tor:
                    assert float((tor[k] - r.v).abs().max()) <= 1e-12 * max(1.0, float(tor[k].abs().max())), (name, k)
                ratio = within(after[k], tor.get(k, r.v), r.e)[1]
                print(f"whole step {case} {'graph' if use_graph else 'eager'} it={it} {name} {k}: error / bound {ratio:.3f}")
                assert ratio <= 1.0, (name, it, k, ratio)
            assert not same_bits(after["param"], b["param"])


def test_default_and_plain_adam_blocks_keep_the_launches_of_ssr_adam_step(monkeypatch):
    """StepConfig without optimizer blocks (what a shipped option file gives) and an explicit plain Adam block: AdamState, and a step
    calls ssr_adam_step_guarded once per network and the new entry points never.  AdamW: the other way round."""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.train_step import AdamState, ESRGANTrainStep, StepConfig
    g_kw, d_kw, g0, d0 = _tiny()
    L = hip.lib()
    calls = {}
    for name in ("ssr_adam_step", "ssr_adam_step_guarded", "ssr_optim_step", "ssr_optim_step_guarded"):
        def counted(*a, _f=getattr(L, name), _n=name):
            calls[_n] = calls.get(_n, 0) + 1
            return _f(*a)
        monkeypatch.setattr(L, name, counted)
    plain = O.normalize_optim("optim_g", dict(type="Adam", lr=1e-4, betas=[0.9, 0.99]))
    adamw = O.normalize_optim("optim_g", dict(type="AdamW", lr=1e-4))
    lr, gt = torch.rand(2, 6, 8, 8).cuda(), torch.rand(2, 3, 32, 32).cuda()
    for cfg, kind, want in ((StepConfig(), AdamState, {"ssr_adam_step_guarded": 2}), (StepConfig(optim_g=plain, optim_d=plain), AdamState, {"ssr_adam_step_guarded": 2}),
                            (StepConfig(optim_g=adamw), None, {"ssr_adam_step_guarded": 1, "ssr_optim_step_guarded": 1})):
        ts = ESRGANTrainStep(g_kw, d_kw, 2, 8, 8, "fp32", cfg, use_graph=False)
        ts.load_state(g0, d0)
        assert type(ts.opt_d) is AdamState and type(ts.opt_g) is (kind or O.OptimState)
        assert isinstance(ts.opt_d.args, hip.AdamArgs)
        calls.clear()
        ts.feed_data(lr, gt)
        ts.step(1)
        torch.cuda.synchronize()
        assert calls == want, calls


# ================================================================================================ the model plugin
def _opt(tmp_path, **train_over):
    from conftest import load_golden
    from test_gpu_boundary import _opt as base_opt
    opt = base_opt(tmp_path, load_golden("step_tiny"), deterministic=True)
    opt["train"].update(train_over)
    return opt


def test_plugin_reports_the_cosine_schedule_over_two_periods(tmp_path):
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.registry import build_model
    sch = {"type": "CosineAnnealingRestartLR", "periods": [4, 6], "restart_weights": [1, 0.5], "eta_min": 1e-7}
    m = build_model(_opt(tmp_path, scheduler=sch, total_iter=11))
    for it in range(1, 12):
        m.update_learning_rate(it)
        want = O.cosine_restart_lr(1e-4, it - 1, [4, 6], [1, 0.5], 1e-7)
        assert m.get_current_learning_rate() == [want], it
        assert m.current_lrs[1] == O.cosine_restart_lr(2e-4, it - 1, [4, 6], [1, 0.5], 1e-7)
    assert m.get_current_learning_rate() == [1e-7]                       # the end of the second period: eta_min
    with pytest.raises(IndexError):
        m.update_learning_rate(12)
    with pytest.raises(ValueError, match="periods"):
        build_model(_opt(tmp_path, scheduler=sch, total_iter=12))


PLUGIN_CASES = {
    "adamw_amsgrad+rmsprop": (dict(type="AdamW", lr=1e-4, betas=[0.9, 0.99], weight_decay=0.01, amsgrad=True),
                              dict(type="RMSprop", lr=2e-4, momentum=0.5, centered=True)),
    "sgd+adam_wd": (dict(type="SGD", lr=1e-3, momentum=0.9, dampening=0.1), dict(type="Adam", lr=2e-4, betas=[0.5, 0.9], weight_decay=0.01)),
}


@pytest.mark.parametrize("case", list(PLUGIN_CASES))
def test_plugin_save_resume_is_bit_identical_and_the_state_loads_into_torch_optim(tmp_path, case):
    """deterministic: true.  Two iterations, save, one more; a fresh model resumed from the files takes the same third iteration:
    parameters, EMA, every state arena and the step counters bit-identical.  A batch of another shape in between carries every arena
    over (_ensure).  The saved optimizer states load into the matching torch.optim classes on the CPU."""
    import copy
    from conftest import load_golden
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd import optimizers as O
    from satlas_super_resolution_amd.registry import build_model
    from satlas_super_resolution_amd.train import resolve_resume
    from test_gpu_boundary import _batch
    data = list(load_golden("step_tiny")["data"]) * 2
    bg, bd = PLUGIN_CASES[case]
    sch = {"type": "CosineAnnealingRestartLR", "periods": [2, 8], "restart_weights": [1, 0.5], "eta_min": 1e-6}
    opt = _opt(tmp_path, optim_g=bg, optim_d=bd, scheduler=sch)
    a = build_model(opt)
    for it in (1, 2):
        a.update_learning_rate(it)
        a.feed_data(_batch(*data[it - 1]))
        a.optimize_parameters(it)
    a.save(0, 2)
    state = torch.load(tmp_path / "states" / "2.state", weights_only=False)
    for sd, block, store in zip(state["optimizers"], (bg, bd), (a.ts.g_store, a.ts.d_store)):
        spec = O.normalize_optim("optim", block)
        plist = [torch.nn.Parameter(store.tensor(k).cpu().clone()) for k in store.offsets]
        topt = getattr(torch.optim, spec["type"])(plist, **{k: v for k, v in spec.items() if k != "type"})
        topt.load_state_dict(sd)
        assert O.state_dict_type(sd) == spec["type"]
        e = sd["state"][len(plist) - 1]
        assert [k for k in e if k != "step"] == O.state_keys(spec) and ("step" in e) == O.has_step(spec)
        if "step" in e:
            assert float(e["step"]) == 2.0
    assert state["schedulers"][0]["periods"] == [2, 8] and state["schedulers"][0]["last_epoch"] == 1
    a.update_learning_rate(3)
    a.feed_data(_batch(*data[2]))
    a.optimize_parameters(3)
    # ---- a fresh model from the files
    opt_b = copy.deepcopy(opt)
    opt_b["path"].update(pretrain_network_g="published/esrgan.pth", param_key_g="params_ema", strict_load_g=True,
                         resume_state=str(tmp_path / "states" / "2.state"))
    state_b = resolve_resume(opt_b, log=lambda m: None)
    b = build_model(opt_b)
    b.resume_training(state_b)
    b.update_learning_rate(3)
    assert b.current_lrs == a.current_lrs
    b.feed_data(_batch(*data[2]))
    b.optimize_parameters(3)
    for oa, ob, sa, sb in ((a.ts.opt_g, b.ts.opt_g, a.ts.g_store, b.ts.g_store), (a.ts.opt_d, b.ts.opt_d, a.ts.d_store, b.ts.d_store)):
        assert same_bits(sa.data, sb.data)
        assert list(oa.arenas) == list(ob.arenas)
        for k in oa.arenas:
            assert same_bits(oa.arenas[k], ob.arenas[k]), k
        spec = oa.spec
        if O.has_step(spec):
            assert int(oa.step.item()) == int(ob.step.item()) == 3
        else:                                                   # SGD keeps no step: a present buffer counts as initialised
            assert int(ob.step.item()) >= 1
    assert same_bits(a.ts.opt_g.ema, b.ts.opt_g.ema)
    # ---- another batch shape: the rebuilt step carries every arena and the counters over
    keep = [{k: t.clone() for k, t in o.arenas.items()} for o in (a.ts.opt_g, a.ts.opt_d)]
    lr, gt = data[3]
    a.feed_data(_batch(lr[:1], gt[:1]))
    assert a.ts.B == 1
    for o, kept in zip((a.ts.opt_g, a.ts.opt_d), keep):
        assert list(o.arenas) == list(kept) and int(o.step.item()) == 3
        for k in kept:
            assert same_bits(o.arenas[k], kept[k]), k
    # ---- a state written by another optimizer type is refused by name
    opt_c = copy.deepcopy(opt_b)
    opt_c["train"]["optim_g"] = dict(type="RMSprop", lr=1e-4)
    c = build_model(opt_c)
    c.resume_training(state_b)
    with pytest.raises(ValueError, match="optim_g"):
        c.feed_data(_batch(*data[2]))
