"""GPU: `tower_attention: mfma` - the blocks' self-attention as ssr_mha_mfma_fwd / ssr_mha_mfma_bwd (csrc/mha_mfma.hip) - through
ClipLossPlan, the train step and the CLIPScore metric, at the gates the FMA path is held to:

  * ClipLossPlan under both tower_arithmetic values on towers A (81 tokens, head dim 64) and B (9 tokens, head dim 72) and both image
    sizes of tests/cliploss_fixture.py against the golden loss and gradient (loss within 1e-4, gradient within 1e-3 max|ref| with no
    element outside), the launch lists, the batch-position and identical-image invariants, and the explicit `fma` against no option;
  * ESRGANTrainStep with the shape and fixture of tests/test_gpu_clip_loss_step.py at that file's tolerances, fp32 and fp32h, and
    hipGraph replay against the eager step;
  * the metric's tower features and pair scores on both tiny towers at the gates of test_tower_features_match_reference and
    test_clipscore_pairs_match_reference (4 x the fp32 CPU deviation of the float64 reference).

The figures these tests printed on an MI355X are in profiles/tower_attention_mfma/observed_errors.txt."""
import copy
import functools
import json
import os

import pytest
import torch

import cliploss_fixture as LF
import clipscore_fixture as FX
from conftest import GOLDEN
from test_gpu_clip_loss import CASES, IDS, _nhwc8

pytestmark = pytest.mark.gpu

ARITHMETICS = ("exact", "split")
DEPTH = 2               # both towers of tests/cliploss_fixture.py


@functools.lru_cache(maxsize=None)
def _golden():
    return LF.load_golden()


@functools.lru_cache(maxsize=None)
def _model(tower, arithmetic="exact", attention="mfma"):
    from satlas_super_resolution_amd.clip_loss import ClipLossModel
    kw = {} if attention is None else {"tower_attention": attention}
    return ClipLossModel(LF.tower_state(tower), "cuda", gelu="tanh", tower_arithmetic=arithmetic, **kw)


def _run(tower, fake, gt, prior=None, weight=LF.LOSS_WEIGHT, arithmetic="exact", attention="mfma"):
    """-> loss scalar (float), grad [N, H, W, 8] on the host, fx, fg, the plan"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.clip_loss import ClipLossPlan
    n, _, h, w = fake.shape
    fb, tb = _nhwc8(fake, 0), _nhwc8(gt, 4)
    grad = (prior.clone() if prior is not None else torch.zeros(n, h, w, 8)).cuda()
    loss = torch.zeros(hip.LOSS_SLOTS, device="cuda")
    plan = ClipLossPlan(_model(tower, arithmetic, attention), n, h, w, hip.View(fb.data_ptr(), 8, 0), hip.View(tb.data_ptr(), 8, 4),
                        hip.View(grad.data_ptr(), 8, 0), loss.data_ptr(), weight, hip.DETERMINISTIC)
    plan.run()
    torch.cuda.synchronize()
    assert bool((loss[1:] == 0).all())
    return float(loss[0]), grad.cpu(), plan.features_fake.cpu().clone(), plan.features_target.cpu().clone(), plan


def _names(plan):
    return [(fn.__name__, what) for fn, _, what in plan.launcher.flat_calls()]


def _fns(launcher):
    return [fn.__name__ for fn, _, _ in launcher.flat_calls()]


@pytest.mark.parametrize("arithmetic", ARITHMETICS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mfma_plan_matches_the_golden_loss_and_gradient(case, arithmetic):
    tower, h, w = case
    c = _golden()["cases"][LF.case_key(tower, h, w)]
    assert c["margin"] >= LF.SIGN_MARGIN
    fake, gt = LF.to_float(c["fake_u8"]), LF.to_float(c["gt_u8"])
    prior = torch.randn(3, h, w, 8, generator=torch.Generator().manual_seed(7)) * 1e-3
    loss, grad, fx, fg, plan = _run(tower, fake, gt, prior, arithmetic=arithmetic)
    loss2, grad2, fx2, fg2, _ = _run(tower, fake, gt, prior, arithmetic=arithmetic)
    el = abs(loss - float(c["loss"])) / float(c["loss"])
    want = c["grad"].permute(0, 2, 3, 1) + prior[..., :3].double()
    ref = float(c["grad"].abs().max())
    delta = (grad[..., :3].double() - want).abs()
    outside = int((delta > 1e-3 * ref).sum())
    print(f"ClipLossPlan mfma / {arithmetic} {tower} {h}x{w}: loss |err| / ref {el:.3e}, gradient max |delta| / max|ref| {float(delta.max()) / ref:.3e}, "
          f"{outside} of {delta.numel()} outside 1e-3")
    assert loss == loss2 and grad.numpy().tobytes() == grad2.numpy().tobytes() and fx.numpy().tobytes() == fx2.numpy().tobytes()
    assert grad[..., 3:].numpy().tobytes() == prior[..., 3:].contiguous().numpy().tobytes()          # the other channels of the gradient image
    # the blocks run the new entries in all three lists; the pooling head keeps the FMA entries, once per pass
    for part in (plan.fwd_target, plan.fwd_fake):
        fns = _fns(part)
        assert fns.count("ssr_mha_mfma_fwd") == DEPTH and fns.count("ssr_mha_fwd") == 1 and "ssr_mha_bwd" not in fns
    fns = _fns(plan.bwd)
    assert fns.count("ssr_mha_mfma_bwd") == DEPTH and fns.count("ssr_mha_bwd") == 1 and "ssr_mha_fwd" not in fns and "ssr_mha_mfma_fwd" not in fns
    whats = dict((what, name) for name, what in _names(plan))
    assert whats["attention pool"] == "ssr_mha_fwd" and whats["attention bwd pool"] == "ssr_mha_bwd"
    assert whats["attention blocks.0"] == "ssr_mha_mfma_fwd" and whats["attention bwd blocks.1"] == "ssr_mha_mfma_bwd"
    assert ("ssr_linear_split" in _fns(plan.launcher)) == (arithmetic == "split") and ("ssr_linear" in _fns(plan.launcher)) == (arithmetic == "exact")
    assert el <= 1e-4
    assert outside == 0


@pytest.mark.parametrize("tower", list(LF.TOWERS))
def test_mfma_feature_bytes_do_not_depend_on_the_batch_position(tower):
    h, w = LF.SIZES[1]
    c = _golden()["cases"][LF.case_key(tower, h, w)]
    fake, gt = LF.to_float(c["fake_u8"]), LF.to_float(c["gt_u8"])
    _, _, fx, fg, _ = _run(tower, fake, gt)
    order = [2, 0, 1]
    _, _, fxp, fgp, _ = _run(tower, fake[order], gt[order])
    assert fxp.numpy().tobytes() == fx[order].contiguous().numpy().tobytes() and fgp.numpy().tobytes() == fg[order].contiguous().numpy().tobytes()
    # the generated rows (saved activations, separate buffers) and the target rows (scratch) run identical arithmetic
    _, _, fa, fb, _ = _run(tower, gt, gt)
    assert fa.numpy().tobytes() == fb.numpy().tobytes() == fg.numpy().tobytes()


@pytest.mark.parametrize("arithmetic", ARITHMETICS)
@pytest.mark.parametrize("tower", list(LF.TOWERS))
def test_mfma_identical_images_give_zero_loss_and_gradient(tower, arithmetic):
    h, w = LF.SIZES[0]
    gt = LF.to_float(_golden()["cases"][LF.case_key(tower, h, w)]["gt_u8"])
    loss, grad, _, _, _ = _run(tower, gt, gt, arithmetic=arithmetic)
    assert loss == 0.0 and bool((grad[..., :3] == 0).all())


def test_the_explicit_option_fma_gives_the_bytes_and_the_launch_list_of_no_option():
    h, w = LF.SIZES[1]
    c = _golden()["cases"][LF.case_key("A", h, w)]
    fake, gt = LF.to_float(c["fake_u8"]), LF.to_float(c["gt_u8"])
    prior = torch.randn(3, h, w, 8, generator=torch.Generator().manual_seed(7)) * 1e-3
    l0, g0, fx0, fg0, p0 = _run("A", fake, gt, prior, attention=None)
    l1, g1, fx1, fg1, p1 = _run("A", fake, gt, prior, attention="fma")
    assert l0 == l1 and g0.numpy().tobytes() == g1.numpy().tobytes() and fx0.numpy().tobytes() == fx1.numpy().tobytes()
    assert fg0.numpy().tobytes() == fg1.numpy().tobytes()
    assert _names(p0) == _names(p1) and not any("mfma" in n for n, _ in _names(p0))
    assert [n for n, _ in _names(p0)].count("ssr_mha_fwd") == 2 * (DEPTH + 1) and [n for n, _ in _names(p0)].count("ssr_mha_bwd") == DEPTH + 1
    assert sorted(p0.model.w) == sorted(p1.model.w) == sorted(_model("A").w)                 # no weight changes with the option
    # and mfma is another order of additions than fma's
    _, _, fxm, _, _ = _run("A", fake, gt, prior)
    assert fxm.numpy().tobytes() != fx0.numpy().tobytes()


def test_a_head_dim_the_entries_do_not_take_is_refused_when_the_plan_is_built():
    from satlas_super_resolution_amd import clipscore_metric as CM
    state = FX.rule_state("clip", 11, width=96, heads=3, mlp=128, depth=1, patch=16, grid=3, out_dim=32)          # heads of 32
    images = FX.fixture_images().cuda()
    assert CM.clip_image_features(images, CM.CLIPVisualModel(state, "cuda")).shape == (3, 32)                     # the FMA path takes it
    with pytest.raises(NotImplementedError, match="calculate_clipscore.*tower_attention 'mfma' takes head dims .*this tower has 32"):
        CM.clip_image_features(images, CM.CLIPVisualModel(state, "cuda", tower_attention="mfma"))


# ------------------------------------------------------------------ through the train step
DATA_SEED = 58          # tests/test_gpu_clip_loss_step.py: chosen so that no sign(fx - fg) can flip; the margin is asserted below


def _setup(tmp_path, weight=None):
    """the setup of tests/test_gpu_clip_loss_step.py with `tower_attention: mfma` in the option block"""
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    path = str(tmp_path / "tower_a.pth")
    torch.save(LF.tower_state("A"), path)
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["cliploss_esrgan_s2naip_urban.yml"]
    opt["feed_disc_lr"] = False
    del opt["train"]["perceptual_opt"]
    opt["train"]["clip_opt"].update(clip_weights=path, tower_attention="mfma")
    if weight is not None:
        opt["train"]["clip_opt"]["loss_weight"] = weight
    cfg = train_config_from_opt(opt)
    assert cfg.clip["tower_attention"] == "mfma" and "tower_arithmetic" not in cfg.clip
    g_kw = dict(num_in_ch=6, num_out_ch=3, scale=4, num_feat=16, num_block=1, num_grow_ch=8)
    d_kw = dict(num_in_ch=3, num_feat=8, skip_connection=True)
    g0, d0 = O.generator_init(seed=41, **g_kw), O.discriminator_init(3, 8, seed=42)
    torch.manual_seed(DATA_SEED)
    lr, gt = torch.rand(2, 6, 16, 16), torch.rand(2, 3, 64, 64)
    return cfg, g_kw, d_kw, g0, d0, lr, gt


def _step(cfg, g_kw, d_kw, g0, d0, lr, gt, dtype="fp32", use_graph=False, iters=(1,)):
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    ts = ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, dtype, cfg, use_graph=use_graph)
    ts.load_state(g0, d0)
    ts.feed_data(lr.cuda(), gt.cuda())
    for it in iters:
        ts.step(it)
    torch.cuda.synchronize()
    return ts


@pytest.mark.parametrize("dtype", ["fp32", "fp32h"])
def test_mfma_step_logs_the_reference_loss_and_adds_its_image_gradient(tmp_path, dtype):
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd.clipscore_metric import vit_config_from_state, vit_features_from_input
    W_ = 0.5
    cfg, g_kw, d_kw, g0, d0, lr, gt = _setup(tmp_path, weight=W_)
    plain_cfg = copy.deepcopy(cfg)
    plain_cfg.clip = None
    ts = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, dtype)
    ts0 = _step(plain_cfg, g_kw, d_kw, g0, d0, lr, gt, dtype)
    assert ts.c_plan is not None and ts.c_plan.model.tower_attention == "mfma" and ts.c_plan.model.tower_arithmetic == "exact" and ts0.c_plan is None
    fns = _fns(ts.c_plan.launcher)
    assert fns.count("ssr_mha_mfma_fwd") == 2 * DEPTH and fns.count("ssr_mha_mfma_bwd") == DEPTH and fns.count("ssr_mha_fwd") == 2
    assert fns.count("ssr_mha_bwd") == 1
    log = ts.log()
    assert ts.fake_in.cpu().numpy().tobytes() == ts0.fake_in.cpu().numpy().tobytes()
    fake = ts.fake_in[..., :3].double().cpu().permute(0, 3, 1, 2).contiguous()
    tgt = ts.l1_tgt[..., :3].double().cpu().permute(0, 3, 1, 2).contiguous()
    sd = LF.tower_state("A")
    size = vit_config_from_state(sd)["image_size"]
    with torch.no_grad():
        fx, fg = (vit_features_from_input(CL.clip_loss_input(t, size, torch.float64), sd, "tanh") for t in (fake, tgt))
    margin = float((fx - fg).abs().min() / fx.abs().max())
    assert margin >= LF.SIGN_MARGIN, margin
    f = fake.clone().requires_grad_(True)
    ref = CL.clip_loss_reference(f, tgt, sd, W_, "tanh", torch.float64)
    ref.backward()
    closed_loss, closed_grad = CL.clip_loss_grad_reference(fake, tgt, sd, W_, "tanh", torch.float64)
    assert abs(float(closed_loss - ref.detach())) <= 1e-9 * float(ref.detach())          # the two references agree (tests/test_clip_loss_host.py)
    assert float((closed_grad - f.grad).abs().max()) <= 1e-9 * float(f.grad.abs().max())
    el = abs(log["l_clip_sim"] - float(ref.detach())) / float(ref.detach())
    got = (ts.grad_l1[..., :3].double() - ts0.grad_l1[..., :3].double()).cpu().permute(0, 3, 1, 2)
    scale = float(f.grad.abs().max())
    delta = (got - f.grad).abs()
    outside = int((delta > 1e-3 * scale).sum())
    print(f"step mfma {dtype}: l_clip_sim {log['l_clip_sim']:.6f} |err| / ref {el:.3e}, sign margin {margin:.2e}, image gradient max |delta| / "
          f"max|ref| {float(delta.max()) / scale:.3e} (max|ref| {scale:.3e}), {outside} outside")
    assert el <= 1e-4
    assert outside == 0
    assert float(ts.grad_l1[..., 3:].abs().max()) == 0.0


def test_mfma_graph_replay_gives_the_eager_steps_bytes(tmp_path):
    """deterministic mode, three iterations: the graph is captured on the second and replayed on the third"""
    cfg, g_kw, d_kw, g0, d0, lr, gt = _setup(tmp_path)
    cfg.deterministic = True
    eager = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, "fp32h", use_graph=False, iters=(1, 2, 3))
    graph = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, "fp32h", use_graph=True, iters=(1, 2, 3))
    assert graph._graphs and graph.c_plan.model.tower_attention == "mfma"
    le, lg = eager.log(), graph.log()
    assert le == lg and lg["l_clip_sim"] > 0
    for a, b in ((eager.g_store.data, graph.g_store.data), (eager.d_store.data, graph.d_store.data), (eager.grad_l1, graph.grad_l1),
                 (eager.opt_g.ema, graph.opt_g.ema)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ------------------------------------------------------------------ through the metric
FEEDS = {"reference": dict(bgr=True, normalize=False), "rgb+normalize": dict(bgr=False, normalize=True)}


@pytest.fixture(scope="module", params=["siglip", "clip"])
def tower(request):
    """a tiny tower as the fixture of tests/test_gpu_clipscore.py builds it: the float64 reference, the gate 4 x the deviation of the
    float32 CPU run of the reference from it over all inputs (nothing of the device in it), and the model with mfma attention"""
    from satlas_super_resolution_amd import clipscore_metric as CM
    family = request.param
    state = FX.tiny_state(family)
    images = FX.fixture_images()
    ref, cpu32, top = {}, 0.0, 0.0
    for feed, kw in FEEDS.items():
        ref[feed] = CM.clip_image_features_reference(state, images, dtype=torch.float64, **kw)
        r32 = CM.clip_image_features_reference(state, images, dtype=torch.float32, **kw).double()
        cpu32, top = max(cpu32, float((r32 - ref[feed]).abs().max())), max(top, float(ref[feed].abs().max()))
    return {"CM": CM, "name": f"{family} tiny", "family": family, "state": state, "images": images, "ref": ref, "cpu32": cpu32, "top": top,
            "gate": 4 * cpu32, "model": CM.CLIPVisualModel(state, "cuda", tower_attention="mfma")}


@pytest.mark.parametrize("feed", list(FEEDS))
def test_mfma_tower_features_match_reference(tower, feed):
    CM, images, want = tower["CM"], tower["images"], tower["ref"][feed]
    fns = _fns(tower["model"].plan(3, 37, 53, **FEEDS[feed]).launcher)
    assert fns.count("ssr_mha_mfma_fwd") == 2 and fns.count("ssr_mha_fwd") == (1 if tower["family"] == "siglip" else 0)
    dev = images.cuda()
    got = CM.clip_image_features(dev, tower["model"], **FEEDS[feed])
    err = float((got.cpu().double() - want).abs().max())
    print(f"tower mfma {tower['name']} / {feed}: device {err / tower['top']:.3e} max|ref| (gate {tower['gate'] / tower['top']:.3e}, "
          f"fp32 CPU {tower['cpu32'] / tower['top']:.3e})")
    again = CM.clip_image_features(dev, tower["model"], **FEEDS[feed])
    assert got.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    assert err <= tower["gate"], (err, tower["gate"])
    gold = FX.load_golden(tower["family"])
    assert float((got.cpu().double() - gold["features"][feed]).abs().max()) <= tower["gate"] + 1e-9 * tower["top"]
    one = CM.clip_image_features(dev[:1], tower["model"], **FEEDS[feed])
    assert one.cpu().numpy().tobytes() == got[:1].cpu().numpy().tobytes()
    three = CM.clip_image_features(torch.cat([dev[1:2], dev[2:3], dev[:1]]), tower["model"], **FEEDS[feed])
    assert three[2:].cpu().numpy().tobytes() == got[:1].cpu().numpy().tobytes() and three[:1].cpu().numpy().tobytes() == got[1:2].cpu().numpy().tobytes()


@pytest.mark.parametrize("feed", list(FEEDS))
def test_mfma_clipscore_pairs_match_reference(tower, feed):
    """the bound of test_clipscore_pairs_match_reference: a feature error of at most e per element moves the score by at most
    2 e sqrt(E) / min|f|"""
    CM, images, ref = tower["CM"], tower["images"].cuda(), tower["ref"][feed]
    a, b = images[:1], images[1:2]
    want = CM.cosine_pairs_reference(ref[:1], ref[1:2])
    got = CM.clipscore(a, b, tower["model"], **FEEDS[feed])
    bound = 2 * tower["gate"] * ref.shape[1] ** 0.5 / float(ref.norm(dim=1).min())
    print(f"clipscore mfma {tower['name']} / {feed}: {float(got[0])!r} against {float(want[0])!r}: |err| {abs(float(got[0] - want[0])):.3e} "
          f"(bound {bound:.3e})")
    assert abs(float(got[0] - want[0])) <= bound
    same = CM.clipscore(a, a, tower["model"], **FEEDS[feed])
    assert abs(1 - float(same[0])) <= 2.0 ** -50


def test_calculate_clipscore_takes_the_option_and_caches_one_model_per_value(tmp_path):
    from satlas_super_resolution_amd import clipscore_metric as CM
    wfile = str(tmp_path / "clip_tiny.pth")
    torch.save(FX.to_openai_clip(FX.tiny_state("clip")), wfile)
    images = FX.fixture_images().cuda()
    kw = dict(clip_model="clip-ViT-B/16", clip_weights=wfile)
    before = len(CM._MODELS)
    fma = CM.calculate_clipscore(images[0], images[1], **kw)
    assert CM.calculate_clipscore(images[0], images[1], tower_attention="fma", **kw) == fma and len(CM._MODELS) == before + 1
    mfma = CM.calculate_clipscore(images[0], images[1], tower_attention="mfma", **kw)
    assert len(CM._MODELS) == before + 2
    assert CM.calculate_clipscore(images[0], images[1], tower_attention="mfma", **kw) == mfma and len(CM._MODELS) == before + 2
    CM.calculate_clipscore(images[0], images[1], tower_attention="mfma", tower_arithmetic="split", **kw)
    assert len(CM._MODELS) == before + 3
    direct = CM.clipscore(images[:1], images[1:2], CM.CLIPVisualModel(FX.tiny_state("clip"), "cuda", tower_attention="mfma"))
    assert mfma == float(direct[0])
    with pytest.raises(NotImplementedError, match="calculate_clipscore.*tower_attention='wmma'"):
        CM.calculate_clipscore(images[0], images[1], tower_attention="wmma", **kw)
