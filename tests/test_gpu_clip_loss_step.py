"""GPU: the CLIP loss inside the train step.  One G + D step on the tiny networks of tests/test_gpu_ssim_loss.py with tower A of
tests/cliploss_fixture.py as `train.clip_opt` (the shipped cliploss_esrgan_s2naip_urban.yml block plus `clip_weights`): the logged
l_clip_sim and the image gradient against clip_loss_reference in float64 on the generator output read back from the device, the log
keys in the reference's order, hipGraph replay against the eager step, and save / resume through the model plugin.

The data seed (58) was chosen on the CPU so that min|fx - fg| >= 1e-3 max|fx| for the oracle's generator output (6.3e-3 there): no
sign(fx - fg) can flip under fp32 rounding; the margin is asserted again on what the device produced."""
import copy
import json
import os

import pytest
import torch

import cliploss_fixture as LF
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DATA_SEED = 58
LOG_ORDER = ["l_g_pix", "l_g_gan", "l_clip_sim", "l_d_real", "out_d_real", "l_d_fake", "out_d_fake"]


def _setup(tmp_path, weight=None):
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    path = str(tmp_path / "tower_a.pth")
    torch.save(LF.tower_state("A"), path)
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["cliploss_esrgan_s2naip_urban.yml"]
    opt["feed_disc_lr"] = False
    del opt["train"]["perceptual_opt"]
    opt["train"]["clip_opt"]["clip_weights"] = path
    if weight is not None:
        opt["train"]["clip_opt"]["loss_weight"] = weight
    cfg = train_config_from_opt(opt)
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
def test_step_logs_the_reference_loss_and_adds_its_image_gradient(tmp_path, dtype):
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd.clipscore_metric import vit_config_from_state, vit_features_from_input
    W_ = 0.5
    cfg, g_kw, d_kw, g0, d0, lr, gt = _setup(tmp_path, weight=W_)
    assert cfg.clip["loss_weight"] == W_ and cfg.perceptual is None and cfg.l1_gt_usm
    plain_cfg = copy.deepcopy(cfg)
    plain_cfg.clip = None
    ts = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, dtype)
    ts0 = _step(plain_cfg, g_kw, d_kw, g0, d0, lr, gt, dtype)
    assert ts.c_plan is not None and ts0.c_plan is None and ts0.clip_loss is None
    log, log0 = ts.log(), ts0.log()
    assert list(log) == LOG_ORDER and list(log0) == [k for k in LOG_ORDER if k != "l_clip_sim"]
    # the same generator forward in both steps: the term is the only difference of grad_l1
    assert ts.fake_in.cpu().numpy().tobytes() == ts0.fake_in.cpu().numpy().tobytes()
    for k in ("l_g_pix", "l_g_gan"):                                          # (block sums arrive in any order outside deterministic mode)
        assert abs(log[k] - log0[k]) <= 1e-6 * abs(log0[k])
    fake = ts.fake_in[..., :3].double().cpu().permute(0, 3, 1, 2).contiguous()
    assert torch.equal(fake.float(), ts.output().cpu())
    tgt = ts.l1_tgt[..., :3].double().cpu().permute(0, 3, 1, 2).contiguous()        # the reference's l1_gt (USM-sharpened here)
    sd = LF.tower_state("A")
    size = vit_config_from_state(sd)["image_size"]
    with torch.no_grad():
        fx, fg = (vit_features_from_input(CL.clip_loss_input(t, size, torch.float64), sd, "tanh") for t in (fake, tgt))
    margin = float((fx - fg).abs().min() / fx.abs().max())
    assert margin >= LF.SIGN_MARGIN, margin
    f = fake.clone().requires_grad_(True)
    ref = CL.clip_loss_reference(f, tgt, sd, W_, "tanh", torch.float64)
    ref.backward()
    el = abs(log["l_clip_sim"] - float(ref.detach())) / float(ref.detach())
    got = (ts.grad_l1[..., :3].double() - ts0.grad_l1[..., :3].double()).cpu().permute(0, 3, 1, 2)
    scale = float(f.grad.abs().max())
    base = float(ts0.grad_l1[..., :3].abs().max())
    delta = (got - f.grad).abs()
    outside = int((delta > 1e-3 * scale).sum())
    print(f"step {dtype}: l_clip_sim {log['l_clip_sim']:.6f} |err| / ref {el:.3e}, sign margin {margin:.2e}, image gradient max |delta| / "
          f"max|ref| {float(delta.max()) / scale:.3e} (max|ref| {scale:.3e}, max|grad_l1| without the term {base:.3e}), {outside} outside")
    assert el <= 1e-4
    assert outside == 0
    assert float(ts.grad_l1[..., 3:].abs().max()) == 0.0
    # the term reaches the generator's parameters
    gk = "conv_last.weight"
    moved = float((ts.g_store.tensor(gk, ts.g_store.grad) - ts0.g_store.tensor(gk, ts0.g_store.grad)).abs().max())
    assert moved > 0


def test_graph_replay_gives_the_eager_steps_bytes(tmp_path):
    """deterministic mode (fixed-order reductions: two runs of the whole step are bit-identical), three iterations: the graph is
    captured on the second and replayed on the third"""
    cfg, g_kw, d_kw, g0, d0, lr, gt = _setup(tmp_path)
    cfg.deterministic = True
    eager = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, "fp32h", use_graph=False, iters=(1, 2, 3))
    graph = _step(cfg, g_kw, d_kw, g0, d0, lr, gt, "fp32h", use_graph=True, iters=(1, 2, 3))
    assert graph._graphs and eager.clip_loss.numel() == graph.clip_loss.numel() > 1            # SSR_LOSS_SLOTS slots in deterministic mode
    le, lg = eager.log(), graph.log()
    assert list(lg) == LOG_ORDER and le == lg and lg["l_clip_sim"] > 0
    assert bool((graph.clip_loss[1:] == 0).all())
    for a, b in ((eager.g_store.data, graph.g_store.data), (eager.d_store.data, graph.d_store.data), (eager.grad_l1, graph.grad_l1),
                 (eager.opt_g.ema, graph.opt_g.ema)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_bf16_and_data_parallel_steps_refuse_the_option(tmp_path):
    from satlas_super_resolution_amd.dp import DPContext
    from satlas_super_resolution_amd.train_step import ESRGANTrainStep
    cfg, g_kw, d_kw, g0, d0, lr, gt = _setup(tmp_path)
    with pytest.raises(NotImplementedError, match="clip_opt.*bf16"):
        ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "bf16", cfg, use_graph=False)
    with pytest.raises(NotImplementedError, match="clip_opt.*world size"):
        ESRGANTrainStep(g_kw, d_kw, 2, 16, 16, "fp32", cfg, dp=DPContext(None, 0, 1, force=True), use_graph=False)


def test_model_plugin_saves_and_resumes_as_without_the_option(tmp_path):
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd.registry import build_model
    wfile = str(tmp_path / "tower_a.pth")
    torch.save(LF.tower_state("A"), wfile)
    base = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["cliploss_esrgan_s2naip_urban.yml"]
    base.update(is_train=True, dist=False, rank=0, world_size=1, compute_dtype="fp32h", manual_seed=3)
    del base["train"]["perceptual_opt"]
    base["network_d"]["num_in_ch"] = 3 + base["network_g"]["num_in_ch"]     # as in test_gpu_boundary: the shipped D width cannot run
    base["network_g"]["num_block"] = 1                                      # the loss plumbing is under test, not the body's depth
    g = torch.Generator().manual_seed(0)
    batch = {"lr": torch.randint(0, 256, (2, 36, 16, 16), generator=g, dtype=torch.uint8),
             "hr": torch.randint(0, 256, (2, 3, 64, 64), generator=g, dtype=torch.uint8)}
    saved = {}
    for tag in ("clip", "plain"):
        opt = json.loads(json.dumps(base))
        opt["path"].update(models=str(tmp_path / tag / "models"), training_states=str(tmp_path / tag / "states"),
                           visualization=str(tmp_path / tag / "vis"))
        if tag == "clip":
            opt["train"]["clip_opt"]["clip_weights"] = wfile
        else:
            del opt["train"]["clip_opt"]
        model = build_model(opt)
        assert (model.cfg.clip is not None) == (tag == "clip")
        model.update_learning_rate(1, warmup_iter=-1)
        model.feed_data(batch)
        model.optimize_parameters(1)
        log = model.get_current_log()
        assert ("l_clip_sim" in log) == (tag == "clip") and list(log)[:2] == ["l_g_pix", "l_g_gan"]
        if tag == "clip":
            assert list(log)[2] == "l_clip_sim" and 0 < log["l_clip_sim"] < float("inf")
        model.save(0, 1)
        files = {n: torch.load(os.path.join(opt["path"]["models"], n), map_location="cpu") for n in ("net_g_1.pth", "net_d_1.pth")}
        state = torch.load(os.path.join(opt["path"]["training_states"], "1.state"), map_location="cpu", weights_only=False)
        saved[tag] = (opt, files, state)
    (oc, fc, sc), (_, fp, sp) = saved["clip"], saved["plain"]
    for n in fc:                                                            # the same files with the same keys and shapes: no tower in a checkpoint
        assert {k: list(fc[n][k]) for k in fc[n]} == {k: list(fp[n][k]) for k in fp[n]}
        assert all(fc[n][k][p].shape == fp[n][k][p].shape for k in fc[n] for p in fc[n][k])
    assert set(sc) == set(sp) and len(sc["optimizers"]) == 2
    assert [len(o["state"]) for o in sc["optimizers"]] == [len(o["state"]) for o in sp["optimizers"]]
    # resume into a model with the option: the optimizer state arrives, the next step runs and logs the term
    ropt = json.loads(json.dumps(oc))
    ropt["path"]["pretrain_network_g"] = os.path.join(oc["path"]["models"], "net_g_1.pth")
    ropt["path"]["pretrain_network_d"] = os.path.join(oc["path"]["models"], "net_d_1.pth")
    model = build_model(ropt)
    model.resume_training(sc)
    model.update_learning_rate(2, warmup_iter=-1)
    model.feed_data(batch)
    assert model.ts.iter == 1 and int(model.ts.opt_g.step.item()) == 1
    model.optimize_parameters(2)
    assert 0 < model.get_current_log()["l_clip_sim"] < float("inf")
