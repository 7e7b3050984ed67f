"""GPU: the device-side non-finite guard.  compute_dtype fp32h runs the forward convolutions on fp16-split operands: an activation
beyond 65504 or a packed weight beyond 64 turns the outputs into NaN.  Checks: the scan kernel against torch.isfinite at every
alignment, the guarded Adam bit for bit against ssr_adam_step, a captured train step that overflows leaving weights / moments / step
counts as they were (one rank and two ranks over gloo), finite runs unchanged by the guard, and inference / validation raising
instead of writing NaN-derived pixels."""
import ctypes as C
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


def _hip():
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    return torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _within_ulp(got, ref, ulps=1):
    return int((_bits(got).long() - _bits(ref).long()).abs().max()) <= ulps


def _scan(*ts):
    hip, L = _hip()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    src = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    ns = (C.c_int64 * len(ts))(*[t.numel() for t in ts])
    hip.check(L.ssr_nonfinite_scan(src, ns, len(ts), flag.data_ptr(), hip.stream_ptr()), "ssr_nonfinite_scan")
    return int(flag.item())


def _g_arena_numel():
    """the generator arena of bench.py's configs[2] (24 input channels, nf 64, 23 blocks): ParamStore's layout"""
    from satlas_super_resolution_amd import engine
    off = 0
    for s in engine.generator_specs(24, 3, 4, 64, 23, 32):
        off = engine.rup(off + s.cout * s.cin * s.k * s.k, 4)
        if s.bias:
            off += engine.rup(s.cout, 4)
    return off


def test_scan_matches_isfinite_at_every_alignment():
    G = _g_arena_numel()
    assert 16_000_000 < G < 17_500_000
    fi = torch.finfo(torch.float32)
    extremes = torch.tensor([fi.max, -fi.max, fi.tiny / 8, -fi.tiny / 8, -0.0, fi.tiny], device="cuda")   # finite: must not trip it
    nan, inf = float("nan"), float("inf")
    for n in (1, 3, 4, 5, 1023, 4099, G):
        for off in ((0, 1, 2, 3) if n < G else (1, 3)):
            buf = torch.randn(n + 8, device="cuda")
            buf[:off] = nan                         # poisoned neighbours: the scan must stay inside its range
            buf[off + n:] = nan
            x = buf[off:off + n]
            k = min(n, extremes.numel())
            x[n - k:] = extremes[:k]
            assert _scan(x) == 0, (n, off)
            for pos in sorted({0, n - 1, max(0, n - 2), n // 2}):      # first, last, inside the scalar tail, the vector body
                old = x[pos].clone()
                for v in (nan, inf, -inf):
                    x[pos] = v
                    assert _scan(x) == int(not bool(torch.isfinite(x).all())) == 1, (n, off, pos, v)
                x[pos] = old
            assert _scan(x) == 0
    a, b = torch.randn(1000, device="cuda"), torch.randn(4099, device="cuda")    # several ranges in one launch
    assert _scan(a, b[1:]) == 0
    b[4098] = nan
    assert _scan(a, b[1:]) == 1 and _scan(a, b[:4097]) == 0


def _adam_tensors(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = {k: torch.randn(n, device="cuda", generator=g) for k in ("param", "grad", "m", "ema")}
    t["v"] = torch.rand(n, device="cuda", generator=g) * 1e-2
    t["lr"] = torch.full((1,), 1e-3, device="cuda")
    t["step"] = torch.full((1,), 4, dtype=torch.int32, device="cuda")
    return t


def _adam_args(hip, t, decay):
    return hip.AdamArgs(t["param"].data_ptr(), t["grad"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["ema"].data_ptr(),
                        t["param"].numel(), t["lr"].data_ptr(), t["step"].data_ptr(), 0.9, 0.99, 1e-8, decay, 0.5)


def test_guarded_adam_is_ssr_adam_step_or_a_skip():
    hip, L = _hip()
    n, decay = 100_003, 0.999
    t0 = _adam_tensors(n, 7)
    plain = {k: v.clone() for k, v in t0.items()}
    guarded = {k: v.clone() for k, v in t0.items()}
    words = torch.zeros(2, dtype=torch.int32, device="cuda")          # flag, skipped
    st = hip.stream_ptr()
    hip.check(L.ssr_adam_step(C.byref(_adam_args(hip, plain, decay)), st), "ssr_adam_step")
    hip.check(L.ssr_adam_step_guarded(C.byref(_adam_args(hip, guarded, decay)), words.data_ptr(), words.data_ptr() + 4, st), "guarded")
    for k in t0:
        assert _same(plain[k], guarded[k]), k                         # flag 0: bit for bit, step 4 -> 5 included
    assert int(guarded["step"].item()) == 5 and words.tolist() == [0, 0]
    skip = {k: v.clone() for k, v in t0.items()}
    words[0] = 1
    hip.check(L.ssr_adam_step_guarded(C.byref(_adam_args(hip, skip, decay)), words.data_ptr(), words.data_ptr() + 4, st), "guarded")
    for k in ("param", "grad", "m", "v", "step"):
        assert _same(skip[k], t0[k]), k
    d = torch.tensor(decay, dtype=torch.float32, device="cuda")
    assert _within_ulp(skip["ema"], t0["ema"] * d + t0["param"] * (1 - d))       # ema = ema*d + p*(1-d) from the unchanged p
    assert not _same(skip["ema"], t0["ema"])
    assert words.tolist() == [0, 1]                                   # flag cleared, one skip counted


# ---------------------------------------------------------------- the train step
def _cfg(fx, det=True):
    from satlas_super_resolution_amd.train_step import StepConfig
    return StepConfig(lr_g=fx["lr"], lr_d=fx["lr"], betas=tuple(fx["betas"]), ema_decay=fx["ema_decay"], deterministic=det)


def _step_of(fx, mode="fp32h", dp=None, B=2):
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    ts = ESRGANTrainStep(fx["g_kwargs"], fx["d_kwargs"], B, 8, 8, mode, _cfg(fx), dp=dp, use_graph=True)
    ts.load_state(fx["g0"], fx["d0"])
    return ts


def _feed(ts, batch, sl=slice(None)):
    ts.feed_data(batch["lr"][sl].cuda().float(), batch["hr"][sl].cuda().float(), scale=1.0 / 255)


def _state(ts):
    out = {"g": ts.g_store.data, "d": ts.d_store.data, "ema": ts.opt_g.ema}
    for name, o in (("g", ts.opt_g), ("d", ts.opt_d)):
        out.update({f"{name}_m": o.exp_avg, f"{name}_v": o.exp_avg_sq, f"{name}_step": o.step})
    for k in ts.d_store.sn_names:
        out[f"u.{k}"], out[f"v.{k}"] = ts.d_store.u[k], ts.d_store.v[k]
    return {k: v.detach().clone().cpu() for k, v in out.items()}


KEPT = ("g", "d", "g_m", "g_v", "g_step", "d_m", "d_v", "d_step")


def test_overflowing_replayed_step_keeps_the_state_and_the_next_step_matches_a_fresh_twin():
    fx = load_golden("stepref_plain")
    data = fx["data"]
    ts = _step_of(fx)
    assert ts.nonfinite_guard
    for it in (1, 2):                      # warm-up, capture
        _feed(ts, data[(it - 1) % len(data)])
        ts.step(it)
    assert "step" in ts._graphs
    before = _state(ts)
    _feed(ts, data[2 % len(data)])
    ts.g_plan.xin[0, 0, 0, 0] = 1.0e5      # one LR sample beyond fp16's range: conv_first's fp16 piece overflows
    ts.step(3)                             # a replay of the captured step
    after = _state(ts)
    assert ts.nonfinite_skips() == (1, 1)
    assert not all(v == v for v in ts.log().values())     # the losses of that step were non-finite
    for k in KEPT:
        assert _same(after[k], before[k]), k
    d = torch.tensor(fx["ema_decay"], dtype=torch.float32)
    assert _within_ulp(after["ema"], before["ema"] * d + before["g"] * (1 - d))
    # the next clean step == the step of a fresh ESRGANTrainStep loaded with the state the skipped step left (as SSRESRGANModel._ensure
    # carries it: parameters and spectral-norm u / v through the state dicts, moments, step counters, EMA)
    twin = _step_of(fx)
    twin.load_state(ts.g_store.state_dict(), ts.d_store.state_dict(), reset_ema=False)
    for o, p in ((twin.opt_g, ts.opt_g), (twin.opt_d, ts.opt_d)):
        o.exp_avg.copy_(p.exp_avg); o.exp_avg_sq.copy_(p.exp_avg_sq); o.step.copy_(p.step)
    twin.opt_g.ema.copy_(ts.opt_g.ema)
    for t in (ts, twin):
        _feed(t, data[3 % len(data)])
        t.step(4)
    a, b = _state(ts), _state(twin)
    for k in a:
        assert _same(a[k], b[k]), k
    assert not _same(a["g"], after["g"]) and ts.nonfinite_skips() == (1, 1) and twin.nonfinite_skips() == (0, 0)


@pytest.mark.parametrize("mode", ["fp32h", "bf16"])
def test_guard_is_transparent_in_finite_runs(monkeypatch, mode):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep, StepConfig
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=1, num_grow_ch=32)
    d_kw = dict(num_in_ch=3, num_feat=64, skip_connection=True)
    g0, d0 = O.generator_init(seed=21, **g_kw), O.discriminator_init(3, 64, seed=22)
    torch.manual_seed(3)
    data = [(torch.rand(2, 24, 32, 32), torch.rand(2, 3, 128, 128)) for _ in range(2)]
    res = {}
    for guard in ("1", "0"):
        monkeypatch.setenv("SSR_NONFINITE_GUARD", guard)
        ts = ESRGANTrainStep(g_kw, d_kw, 2, 32, 32, mode, StepConfig(ema_decay=0.999, deterministic=True), use_graph=True)
        assert ts.nonfinite_guard == (guard == "1")
        ts.load_state(g0, d0)
        for it in range(1, 5):             # eager, capture, two replays
            lr, gt = data[it % 2]
            ts.feed_data(lr.cuda(), gt.cuda())
            ts.step(it)
        res[guard] = (_state(ts), dict(ts.log()), ts.nonfinite_skips())
        del ts
    (sa, la, ka), (sb, lb, kb) = res["1"], res["0"]
    for k in sa:
        assert _same(sa[k], sb[k]), (mode, k)
    assert la == lb and ka == kb == (0, 0)


def _plugin_opt(tmp_path, fx):
    return {
        "model_type": "SSRESRGANModel", "scale": 4, "manual_seed": 0, "is_train": True, "dist": False, "name": "t",
        "compute_dtype": "fp32h", "l1_gt_usm": False, "percep_gt_usm": False, "gan_gt_usm": False, "feed_disc_lr": False,
        "network_g": dict(type="SSR_RRDBNet", **fx["g_kwargs"]),
        "network_d": dict(type="SSR_UNetDiscriminatorSN", **fx["d_kwargs"]),
        "path": {"models": str(tmp_path / "models"), "training_states": str(tmp_path / "states"), "visualization": str(tmp_path / "vis")},
        "train": {"ema_decay": fx["ema_decay"], "optim_g": {"type": "Adam", "lr": fx["lr"], "weight_decay": 0, "betas": list(fx["betas"])},
                  "optim_d": {"type": "Adam", "lr": fx["lr"], "weight_decay": 0, "betas": list(fx["betas"])},
                  "pixel_opt": {"type": "L1Loss", "loss_weight": 1.0, "reduction": "mean"},
                  "gan_opt": {"type": "GANLoss", "gan_type": "vanilla", "real_label_val": 1.0, "fake_label_val": 0.0, "loss_weight": 0.1},
                  "net_d_iters": 1, "net_d_init_iters": 0},
    }


def test_plugin_overflow_raises_keeps_weights_and_checkpoint_and_counts_the_skip(tmp_path):
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    fx = load_golden("stepref_plain")
    m = build_model(_plugin_opt(tmp_path, fx))
    m.feed_data(fx["data"][0])
    m.optimize_parameters(1)
    assert all(v == v for v in m.get_current_log().values()) and m.nonfinite_skips == {"net_g": 0, "net_d": 0}
    g_before, d_before = m.ts.g_store.state_dict(), m.ts.d_store.state_dict()
    m.feed_data(fx["data"][1 % len(fx["data"])])
    m.ts.g_plan.xin[0, 0, 0, 0] = 1.0e5
    m.optimize_parameters(2)
    with pytest.raises(FloatingPointError, match="fp32f"):
        m.get_current_log()
    assert m.nonfinite_skips == {"net_g": 1, "net_d": 1}
    for k, v in m.ts.g_store.state_dict().items():
        assert _same(v, g_before[k]) and bool(torch.isfinite(v).all()), k
    for k, v in m.ts.d_store.state_dict().items():
        if not (k.endswith("_u") or k.endswith("_v")):                # (u / v: advanced by the power iterations of the forwards)
            assert _same(v, d_before[k]), k
        assert bool(torch.isfinite(v).all()), k
    m.save(0, 2)
    ck = torch.load(tmp_path / "models" / "net_g_2.pth", weights_only=False)
    for k, v in ck["params"].items():
        assert _same(v, g_before[k]), k
    assert all(bool(torch.isfinite(v).all()) for v in ck["params_ema"].values())
    st = torch.load(tmp_path / "states" / "2.state", weights_only=False)
    assert [float(o["state"][0]["step"]) for o in st["optimizers"]] == [1.0, 1.0]    # applied updates only


# ---------------------------------------------------------------- inference and validation
def _bad_checkpoint(tmp_path):
    from oracle import make_infer_golden as M
    sd = dict(M.write_weights(str(tmp_path / "good.pth")))
    w = sd["conv_first.weight"].clone()
    w.view(-1)[0] = 100.0                  # beyond fp32h's packed-weight range (|w| < 64)
    sd["conv_first.weight"] = w
    torch.save({"params_ema": sd, "params": sd}, tmp_path / "bad.pth")
    return M, sd, str(tmp_path / "bad.pth")


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def test_inference_and_validation_refuse_non_finite_outputs(tmp_path):
    import yaml
    from PIL import Image
    from satlas_super_resolution_amd.infer import run_infer
    from satlas_super_resolution_amd.infer_grid import run_infer_grid
    M, sd, bad = _bad_checkpoint(tmp_path)
    for k in range(3):
        for d, img in ((tmp_path / "single" / "a", M.chunk_image(7, k, 3)), (tmp_path / "grid" / "t1", M.chunk_image(1, 0, k))):
            os.makedirs(d, exist_ok=True)
            Image.fromarray(img).save(d / (f"{k}.png" if "single" in str(d) else f"0_{k}.png"))

    def opt(which, out, dtype):
        o = yaml.safe_load(M.option_text(str(tmp_path / which) + "/", str(tmp_path / out) + "/", bad))
        o["compute_dtype"] = dtype
        return o

    with pytest.raises(FloatingPointError, match="fp32f"):
        run_infer(opt("single", "o_single", "fp32h"))
    with pytest.raises(FloatingPointError, match="fp32f") as e:
        run_infer_grid(opt("grid", "o_grid", "fp32h"))
    assert "t1" in str(e.value)                                       # names the tile of the batch
    assert not _pngs(str(tmp_path / "o_grid")) and not [p for p in _pngs(str(tmp_path / "o_single")) if p.endswith("sr.png")]
    assert run_infer(opt("single", "f_single", "fp32f")) == {"images": 3}                 # the same checkpoint in exact fp32
    assert len([p for p in _pngs(str(tmp_path / "f_single")) if p.endswith("sr.png")]) == 3
    assert run_infer_grid(opt("grid", "f_grid", "fp32f"))["chunks"] == 3
    assert _pngs(str(tmp_path / "f_grid")) == [f"t1/0_{k}.png" for k in range(3)]
    # nondist_validation (test.py's generator-only model) with the same weights
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    vopt = {"model_type": "SSRESRGANModel", "scale": 4, "manual_seed": 0, "is_train": False, "dist": False, "name": "v",
            "compute_dtype": "fp32h", "network_g": dict(type="SSR_RRDBNet", num_in_ch=3, num_out_ch=3, **M.G_KW),
            "path": {"pretrain_network_g": bad, "param_key_g": "params", "strict_load_g": True, "visualization": str(tmp_path / "vis")},
            "val": {"metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": False}}}}

    class DS:
        opt = {"name": "val"}

    class Loader(list):
        dataset = DS()

    lr = torch.from_numpy(M.chunk_image(7, 0, 3)).permute(2, 0, 1)[None].contiguous()
    batch = {"lr": lr, "hr": lr.repeat_interleave(4, 2).repeat_interleave(4, 3)}
    with pytest.raises(FloatingPointError, match="fp32f"):
        build_model(vopt).nondist_validation(Loader([batch]), 1, None, False)
    vopt["compute_dtype"] = "fp32f"
    assert set(build_model(vopt).nondist_validation(Loader([batch]), 1, None, False)) == {"psnr"}


# ---------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from satlas_super_resolution_amd.dp import init_distributed
    ctx = init_distributed(backend="gloo")
    fx = torch.load(os.path.join(GOLDEN, "stepref_plain.pt"), map_location="cpu", weights_only=False)
    ts = _step_of(fx, dp=ctx, B=1)
    ts.sync_params_from_rank0()
    data = fx["data"]
    for it in (1, 2):
        _feed(ts, data[(it - 1) % len(data)], slice(rank, rank + 1))
        ts.step(it)
    before = _state(ts)
    _feed(ts, data[2 % len(data)], slice(rank, rank + 1))
    if rank == 0:                          # only one rank overflows: its NaN reaches the other through the gradient exchange
        ts.g_plan.xin[0, 0, 0, 0] = 1.0e5
    ts.step(3)
    torch.cuda.synchronize()
    torch.save((rank, before, _state(ts), ts.nonfinite_skips()), os.path.join(outdir, f"rank{rank}.pt"))
    ctx.barrier()
    torch.distributed.destroy_process_group()


def test_dp_two_ranks_skip_together_when_one_overflows(tmp_path):
    world, port = 2, _free_port()
    mpc = mp.get_context("spawn")
    procs = [mpc.Process(target=_dp_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    for p in procs:
        if p.is_alive():
            p.kill()
            raise AssertionError("a rank did not finish")
        assert p.exitcode == 0
    res = [torch.load(tmp_path / f"rank{r}.pt", weights_only=False) for r in range(world)]
    for rank, before, after, skips in res:
        assert skips == (1, 1), (rank, skips)
        for k in KEPT:
            assert _same(after[k], before[k]), (rank, k)
    for k in res[0][2]:
        assert _same(res[0][2][k], res[1][2][k]), k
