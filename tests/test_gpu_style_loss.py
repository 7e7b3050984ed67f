"""GPU: the Gram-matrix style term of the VGG19 perceptual loss (style_weight > 0, criterion 'l1'; csrc/gram.hip, perceptual.py):
the Gram kernels against float64, the plan's style loss and feature gradients against a restatement built on the oracle's VGG19
features, the train step with the shipped loss block plus a style weight, run-to-run determinism and the model plugin's log."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LW_WEIGHTS = {"conv1_2": 0.1, "conv2_2": 0.1, "conv3_4": 1, "conv4_4": 1, "conv5_4": 1}       # esrgan_s2naip_urban.yml:125-131
# (C, h, w) of the five taps of a 128 x 128 and of a 32 x 48 image
TAPS_128 = [(64, 128, 128), (128, 64, 64), (256, 32, 32), (512, 16, 16), (512, 8, 8)]
TAPS_32x48 = [(64, 32, 48), (128, 16, 24), (256, 8, 12), (512, 4, 6), (512, 2, 3)]


def _features(B, P, C, tdt, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, P, C, generator=g)
    f[torch.rand(B, P, C, generator=g) < 0.2] = 0.0          # exact zeros (post-ReLU-like) beside negatives
    return f.to(tdt)


def _gram64(f):
    """float64 Gram of NHWC-flat features [B, P, C]: F^T F / (C P)"""
    f = f.double()
    return torch.einsum("npc,npd->ncd", f, f) / (f.shape[1] * f.shape[2])


def _gram_dev(f_dev, dt):
    from satlas_super_resolution_amd import hip
    B, P, C = f_dev.shape
    L = hip.lib()
    s = L.ssr_gram_splits(B, P, C)
    assert s >= 1
    ws = torch.zeros(max(1, s * B * C * C) if s > 1 else 1, device="cuda")
    g = torch.full((B, C, C), float("nan"), device="cuda")
    hip.check(L.ssr_gram_fwd(hip.view(f_dev), g.data_ptr(), ws.data_ptr(), dt, B, P, C, 1.0 / (C * P), hip.stream_ptr()), "ssr_gram_fwd")
    return g, s


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("B,taps", [(2, TAPS_128), (2, TAPS_32x48), (32, TAPS_128[:1])], ids=["B2-128", "B2-32x48", "B32-conv1_2"])
def test_gram_forward_matches_float64(mode, B, taps):
    from satlas_super_resolution_amd import hip
    dt = hip.dtype_code(mode)
    tdt = hip.torch_dtype(dt)
    tol = 1e-5 if mode == "fp32" else 1e-4
    for C, h, w in taps:
        f = _features(B, h * w, C, tdt, seed=C + h)
        g, splits = _gram_dev(f.cuda(), dt)
        if B == 32:
            assert splits > 1                              # the long-K tap of the batch really splits
        ref = _gram64(f)
        got = g.double().cpu()
        assert torch.equal(got, got.transpose(1, 2)), "G must be exactly symmetric"
        for n in range(B):
            err = float((got[n] - ref[n]).abs().max() / ref[n].abs().max())
            assert err <= tol, (mode, C, h, w, n, err, splits)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_gram_loss_sign_and_backward(mode):
    from satlas_super_resolution_amd import hip
    dt = hip.dtype_code(mode)
    tdt = hip.torch_dtype(dt)
    L = hip.lib()
    B = 2
    for C, h, w in TAPS_32x48 + [TAPS_128[0]]:
        P = h * w
        fx, ft = _features(B, P, C, tdt, seed=1 + C), _features(B, P, C, tdt, seed=2 + C)
        fx_d, ft_d = fx.cuda(), ft.cuda()
        gx, _ = _gram_dev(fx_d, dt)
        gt, _ = _gram_dev(ft_d, dt)
        sgn = torch.full((B, C, C), 7.0, dtype=tdt, device="cuda")
        loss = torch.zeros(1, device="cuda")
        wgt = 0.5 / (B * C * C)
        hip.check(L.ssr_gram_l1(gx.data_ptr(), gt.data_ptr(), sgn.data_ptr(), dt, B * C * C, wgt, loss.data_ptr(), hip.stream_ptr()), "l1")
        d_ref = _gram64(fx) - _gram64(ft)
        scale = float(torch.maximum(_gram64(fx).abs().max(), _gram64(ft).abs().max()))
        s_dev = sgn.double().cpu()
        assert torch.equal(s_dev, s_dev.transpose(1, 2))
        sure = d_ref.abs() > 4e-5 * scale                        # outside rounding of zero: the sign is decided
        assert torch.equal(s_dev[sure], torch.sign(d_ref)[sure]), (C, h, w)
        assert bool(((s_dev == 1) | (s_dev == -1) | (s_dev == 0)).all())
        l_ref = 0.5 * float(d_ref.abs().mean())
        assert abs(float(loss) - l_ref) <= 1e-4 * l_ref + 1e-5 * scale, (float(loss), l_ref)
        # backward from the device's own F and sign matrix, accumulating into an old gradient
        coef = 1.0 / C
        old = (0.01 * torch.randn(B, P, C, generator=torch.Generator().manual_seed(C))).to(tdt)
        gf = old.cuda()
        hip.check(L.ssr_gram_bwd(hip.view(fx_d), sgn.data_ptr(), hip.view(gf), dt, B, P, C, coef, 1, hip.stream_ptr()), "bwd")
        ref = old.double() + coef * torch.bmm(fx.double(), s_dev)
        got = gf.double().cpu()
        if mode == "fp32":
            assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), (C, h, w)
        else:
            from oracle.layerwise import bf16_ulp
            # one bf16 ulp of the stored value; below 1e-5 of max|ref| (cancellation to near zero) fp32 summation noise may exceed it
            slack = 1e-5 * float(ref.abs().max())
            assert bool(((got - ref).abs() <= bf16_ulp(ref.abs().float()).double() * 1.0001 + slack).all()), (C, h, w)
        # overwrite mode (perceptual_weight 0: no feature-L1 gradient in the buffer)
        hip.check(L.ssr_gram_bwd(hip.view(fx_d), sgn.data_ptr(), hip.view(gf), dt, B, P, C, coef, 0, hip.stream_ptr()), "bwd")
        ref0 = coef * torch.bmm(fx.double(), s_dev)
        assert float((gf.double().cpu() - ref0).abs().max()) <= (1e-5 if mode == "fp32" else 8e-3) * float(ref0.abs().max())


def _style_ref(fx, ft, layer_weights, sw):
    """BasicSR PerceptualLoss's style term (criterion l1) in float64 from feature dicts (NCHW)"""
    tot = 0.0
    for k, w in layer_weights.items():
        a, b = fx[k].double(), ft[k].double()
        n, c, h, ww = a.shape
        ga = torch.bmm(a.view(n, c, -1), a.view(n, c, -1).transpose(1, 2)) / (c * h * ww)
        gb = torch.bmm(b.view(n, c, -1), b.view(n, c, -1).transpose(1, 2)) / (c * h * ww)
        tot += float((ga - gb).abs().mean()) * w
    return tot * sw


@pytest.mark.parametrize("mode", ["fp32", "fp32h", "bf16"])
@pytest.mark.parametrize("pw", [1.0, 0.0])
def test_perceptual_plan_style_term(mode, pw):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.perceptual import PerceptualPlan
    B, H, W = 2, 32, 48
    sw = 50.0
    sd = O.vgg19_init(seed=3)
    g = torch.Generator().manual_seed(4)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    torch.manual_seed(5)
    x, gt = 0.2 + 0.5 * torch.rand(B, 3, H, W), torch.rand(B, 3, H, W)          # unlike statistics: Grams far apart
    dt = hip.dtype_code(mode)
    tdt = hip.torch_dtype(dt)
    nhwc = lambda t: F.pad(t.permute(0, 2, 3, 1), (0, 5)).contiguous().to(tdt).cuda()
    xb, tb = nhwc(x), nhwc(gt)
    gbuf = torch.zeros_like(xb)
    loss = torch.zeros(2, device="cuda")
    opt = {"type": "PerceptualLoss", "layer_weights": LW_WEIGHTS, "vgg_type": "vgg19", "use_input_norm": True, "perceptual_weight": pw,
           "style_weight": sw, "range_norm": False, "criterion": "l1"}
    plan = PerceptualPlan(opt, B, H, W, dt, xb, tb, gbuf, loss.data_ptr(), state=sd, style_loss_ptr=loss.data_ptr() + 4)
    assert plan.style and plan.feature == (pw > 0)
    plan.pack()
    plan.fwd_target.run()
    plan.fwd.run()
    plan.bwd.run()
    torch.cuda.synchronize()
    prec = O.BF16 if mode == "bf16" else O.FP32
    fx = O.vgg19_features(sd, prec.a(x), LW_WEIGHTS.keys(), prec=prec)
    ft = O.vgg19_features(sd, prec.a(gt), LW_WEIGHTS.keys(), prec=prec)
    ltol = 5e-3 if mode == "bf16" else 1e-4
    s_ref = _style_ref(fx, ft, LW_WEIGHTS, sw)
    assert abs(float(loss[1]) - s_ref) <= ltol * abs(s_ref), (float(loss[1]), s_ref)
    if pw > 0:
        p_ref = float(O.perceptual_loss(sd, prec.a(x), prec.a(gt), LW_WEIGHTS, pw, prec=prec))
        assert abs(float(loss[0]) - p_ref) <= ltol * abs(p_ref), (float(loss[0]), p_ref)
    else:
        assert float(loss[0]) == 0.0                           # no feature term launched
    # feature gradients of the tapped layers, layer-local from the device's own buffers: feature-L1 part (pw > 0), style part
    # from the device's Fx and sign matrix, plus (below the last tap) what the dgrad chain routed back through ReLU + pooling
    from oracle import layerwise as LW
    lmode = "bf16" if mode == "bf16" else "fp32"
    nchw = lambda t: t.float().cpu().permute(0, 3, 1, 2)
    rep = LW.Report()
    last = plan.layers[-1][0]
    for k, w in LW_WEIGHTS.items():
        a = plan.acts[k].double().cpu()                        # [B, h, w, C]
        ft_dev = plan.feats_t[k].double().cpu()
        n, hh, ww, c = a.shape
        s_dev = plan.gram_s[k].double().cpu()
        gram = lambda f: torch.bmm(f.view(n, -1, c).transpose(1, 2), f.view(n, -1, c)) / (c * hh * ww)
        d_ref = gram(a) - gram(ft_dev)
        sure = d_ref.abs() > 4e-5 * max(float(gram(a).abs().max()), float(gram(ft_dev).abs().max()))
        assert torch.equal(s_dev[sure], torch.sign(d_ref)[sure]), k
        style = sw * w / (n * c * c) * 2.0 / (c * hh * ww) * torch.bmm(a.view(n, -1, c), s_dev).view(n, hh, ww, c)
        # in the device's order of storage roundings: feature L1 written, style part added, routed gradient added
        want = style.permute(0, 3, 1, 2)
        if pw > 0:
            want = want + LW.rnd(pw * w * torch.sign(a - ft_dev) / a.numel(), lmode).permute(0, 3, 1, 2)
        want = LW.rnd(want.float(), lmode)
        if k != last:
            f = nchw(plan.acts[k]).requires_grad_(True)
            (routed,) = torch.autograd.grad(F.max_pool2d(F.relu(f), 2, 2), f, nchw(plan.g_pooled[k]))
            want = LW.rnd(want + routed, lmode)
        rep.add(f"g_feat {k}", nchw(plan.g_acts[k]), want)
    if mode == "bf16":
        # the style part is stored (one rounding) before the routed gradient is added: one ulp of that intermediate can be two
        # of a sum that cancels to a smaller binade
        rep.check_bf16(max_ulps=2.0)
    else:
        rep.check(1e-4 if mode == "fp32" else 2e-4, 1e-5)


def _gram_t(f):
    n, c, h, w = f.shape
    v = f.reshape(n, c, h * w)
    return v.bmm(v.transpose(1, 2)) / (c * h * w)


def _with_style(monkeypatch, sw):
    """oracle.esrgan_oracle.perceptual_loss + BasicSR's style term (criterion l1), patched in for the duration of a test"""
    from oracle import esrgan_oracle as O
    orig = O.perceptual_loss

    def wrapped(vgg_sd, x, gt, layer_weights, perceptual_weight=1.0, use_input_norm=True, range_norm=False, prec=O.FP32):
        loss = orig(vgg_sd, x, gt, layer_weights, perceptual_weight, use_input_norm, range_norm, prec)
        fx = O.vgg19_features(vgg_sd, x, layer_weights.keys(), use_input_norm, range_norm, prec)
        with torch.no_grad():
            fg = O.vgg19_features(vgg_sd, gt.detach(), layer_weights.keys(), use_input_norm, range_norm, prec)
        style = 0
        for k, w in layer_weights.items():
            style = style + F.l1_loss(_gram_t(fx[k]), _gram_t(fg[k])) * w
        return loss + style * sw
    monkeypatch.setattr(O, "perceptual_loss", wrapped)


STYLE_W = 100.0


def _tiny_step_setup(style_weight):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]
    opt["feed_disc_lr"] = False
    opt["train"]["perceptual_opt"]["style_weight"] = style_weight
    cfg = step_config_from_opt(opt)
    g_kw = dict(num_in_ch=6, num_out_ch=3, scale=4, num_feat=16, num_block=1, num_grow_ch=8)
    d_kw = dict(num_in_ch=3, num_feat=8, skip_connection=True)
    g0, d0 = O.generator_init(seed=41, **g_kw), O.discriminator_init(3, 8, seed=42)
    vgg = O.vgg19_init(seed=43)
    torch.manual_seed(44)
    lr, gt = torch.rand(2, 6, 16, 16), torch.rand(2, 3, 64, 64)
    return cfg, g_kw, d_kw, g0, d0, vgg, lr, gt


def test_train_step_with_shipped_loss_block_and_style_weight_matches_oracle(monkeypatch):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, vgg, lr, gt = _tiny_step_setup(STYLE_W)
    assert cfg.perceptual["style_weight"] == STYLE_W and cfg.perceptual.get("criterion", "l1") == "l1"
    ocfg = lambda c: O.StepConfig(l1_weight=c.l1_weight, gan_weight=c.gan_weight, lr_g=c.lr_g, lr_d=c.lr_d, betas=c.betas,
                                  ema_decay=c.ema_decay, l1_gt_usm=True, gan_gt_usm=False, percep_gt_usm=True, perceptual=c.perceptual)
    plain = O.ESRGANOracle(g0, d0, ocfg(cfg), vgg_sd=vgg)
    plain.step(lr, gt, 1)
    _with_style(monkeypatch, STYLE_W)
    orc = O.ESRGANOracle(g0, d0, ocfg(cfg), vgg_sd=vgg)
    ref_log = orc.step(lr, gt, 1)
    # the style term matters: some generator gradient moves by far more than the gate below
    moved = max(float((orc.g_grads[k] - plain.g_grads[k]).abs().max() / orc.g_grads[k].abs().max()) for k in orc.g_grads)
    assert moved > 10 * 2e-3, moved
    ts = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32", cfg, use_graph=False, vgg_state=vgg)
    ts.load_state(g0, d0)
    ts.feed_data(lr.cuda(), gt.cuda())
    ts.step(1)
    log = ts.log()
    assert set(log) == set(ref_log) | {"l_g_style"} and log["l_g_style"] > 0
    for k, v in ref_log.items():
        got = log[k] + log["l_g_style"] if k == "l_g_percep" else log[k]
        assert abs(got - v) <= 1e-3 * max(1.0, abs(v)), (k, got, v)
    for k, g in orc.g_grads.items():
        got = ts.g_store.tensor(k, ts.g_store.grad)
        gc_, gr_ = got.detach().float().cpu(), g.detach().float().cpu()
        err, scale = (gc_ - gr_).abs(), float(gr_.abs().max())
        outside = int((err > 2e-3 * (scale + gr_.abs())).sum())
        assert outside <= max(3, int(2e-3 * err.numel())) and float(err.max()) <= 1e-2 * scale and float(err.mean()) <= 1e-3 * scale, \
            (k, outside, err.numel(), float(err.max()) / scale)
    # hipGraph replay of the same step
    ts2 = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32", cfg, use_graph=True, vgg_state=vgg)
    ts2.load_state(g0, d0)
    ts2.feed_data(lr.cuda(), gt.cuda())
    for it in (1, 2, 3):
        ts2.step(it)
    log2 = ts2.log()
    assert "l_g_style" in log2 and all(v == v and abs(v) != float("inf") for v in log2.values())


def test_style_term_is_deterministic_in_fp32h():
    """deterministic mode, fp32h, a batch at which the long taps' Gram launches split over the pixels: two runs from the same state
    give the same bytes"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, vgg, lr, gt = _tiny_step_setup(STYLE_W)
    cfg.deterministic = True
    B = 4
    lr, gt = lr.repeat(2, 1, 1, 1), gt.repeat(2, 1, 1, 1)
    assert hip.lib().ssr_gram_splits(B, 64 * 64, 64) > 1
    runs = []
    for _ in range(2):
        ts = ESRGANTrainStep(g_kw, d_kw, B, 16, 16, "fp32h", cfg, use_graph=True, vgg_state=vgg)
        ts.load_state(g0, d0)
        ts.feed_data(lr.cuda(), gt.cuda())
        for it in (1, 2):
            ts.step(it)
        log = ts.log()
        runs.append((log["l_g_style"], ts.output().cpu(), ts.g_store.data.detach().cpu().clone()))
    assert runs[0][0] == runs[1][0] and runs[0][0] > 0
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


def test_model_plugin_logs_style_loss(tmp_path, monkeypatch):
    from satlas_super_resolution_amd import models, perceptual as P  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["esrgan_s2naip_urban.yml"]
    opt.update(is_train=True, dist=False, rank=0, world_size=1, compute_dtype="fp32h")
    opt["path"].update(models=str(tmp_path / "models"), training_states=str(tmp_path / "states"), visualization=str(tmp_path / "vis"))
    opt["network_d"]["num_in_ch"] = 3 + opt["network_g"]["num_in_ch"]     # as in test_gpu_boundary: the shipped D width cannot run
    opt["network_g"]["num_block"] = 2                                     # the loss plumbing is under test, not the body's depth
    opt["train"]["perceptual_opt"]["style_weight"] = 1.0
    wfile = tmp_path / "vgg19-dcbb9e9d.pth"
    torch.save(P.vgg19_random_state(P.vgg19_specs("conv5_4"), seed=1), wfile)
    monkeypatch.setenv("SSR_VGG19_WEIGHTS", str(wfile))
    model = build_model(json.loads(json.dumps(opt)))
    g = torch.Generator().manual_seed(0)
    for it in (1, 2):
        model.update_learning_rate(it, warmup_iter=-1)
        model.feed_data({"lr": torch.randint(0, 256, (2, 36, 32, 32), generator=g, dtype=torch.uint8),
                         "hr": torch.randint(0, 256, (2, 3, 128, 128), generator=g, dtype=torch.uint8)})
        model.optimize_parameters(it)
    log = model.get_current_log()
    assert set(log) == {"l_g_pix", "l_g_percep", "l_g_style", "l_g_gan", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"}
    assert log["l_g_style"] > 0 and log["l_g_style"] == log["l_g_style"] and log["l_g_style"] != float("inf")
    bad = json.loads(json.dumps(opt))
    bad["train"]["perceptual_opt"]["criterion"] = "l2"
    with pytest.raises(NotImplementedError, match="criterion"):
        m = build_model(bad)
        m.feed_data({"lr": torch.zeros(2, 36, 32, 32, dtype=torch.uint8), "hr": torch.zeros(2, 3, 128, 128, dtype=torch.uint8)})
        m.optimize_parameters(1)
