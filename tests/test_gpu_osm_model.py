"""GPU: the recorded step of the reference's OSMObjESRGANModel (tools/make_osm_model_golden.py: its own feed_data and
optimize_parameters on the CPU) through OSMObjESRGANModel.feed_data / optimize_parameters here, in fp32 and fp32h, with both settings
of osm_obj_resize_antialias; then the step's own properties: graph against eager, save / resume, the checkpoint layout, refusals.

Gates: the crops within the exact-fp32 gate 2e-6 * max|ref| (README, "exact forms") - the real image's against the record, the
generated image's against the float64 statement over the step's OWN output (the record's generated crops carry the generator's
distance, so they are held to the project's gate instead).  Every loss_dict entry, every parameter gradient, the output and the
parameters after the step within the project's 1e-3 * max|ref| gate with 0 elements outside (the record's float32 run is within 1e-4
of its float64 run on each of them: tests/test_osm_model_host.py).  key_conv.bias has a gradient that is zero in exact arithmetic and
is excluded from the relative gate, as the discriminator fixture documents: it is held to 1e-3 * max|gradient of key_conv.weight|."""
import os
import random

import pytest
import torch

import osm_model_fixture as mfx

pytestmark = pytest.mark.gpu

GATE, CROP_GATE = 1e-3, 2e-6
MODES = ("fp32", "fp32h")


@pytest.fixture(scope="module")
def heads():
    return [mfx.load(0), mfx.load(1)]


def _model(head, tmp, mode="fp32", deterministic=False):
    import satlas_super_resolution_amd.models  # noqa: F401  (discovers every *_model.py, as the training loop's import does)
    from satlas_super_resolution_amd.registry import MODEL_REGISTRY
    return MODEL_REGISTRY.get("OSMObjESRGANModel")(mfx.model_opt(head, tmp, mode, deterministic))


def _outside(a, ref, gate=GATE):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    bound = gate * float(ref.abs().max())
    err = (a - ref).abs()
    return int((err > bound).sum()), float(err.max()), bound


def _grads(ts):
    g = {k: ts.g_store.tensor(k, ts.g_store.grad).clone() for k in ts.g_store.offsets}
    d = {k: st.tensor(k, st.grad).clone() for st, k in ts.d_param_slots()}
    return g, d


@pytest.mark.parametrize("aa", (0, 1))
@pytest.mark.parametrize("mode", MODES)
def test_recorded_step(heads, tmp_path, mode, aa):
    from satlas_super_resolution_amd import osm_reference as R
    head = heads[aa]
    m = _model(head, tmp_path, mode)
    random.seed(head["seed"])
    m.feed_data(mfx.batch_of(head))
    assert m.chosen == head["chosen"] and random.random() == head["random_after"]
    ts = m.ts
    assert ts.antialias == bool(aa) and ts.Bo == 4
    real = ts.object_crops("real")
    n, err, bound = _outside(real, head["crops_gt"], CROP_GATE)
    print(f"{mode} aa{aa} real crops: max err {err:.3e} bound {bound:.3e}")
    assert n == 0
    m.optimize_parameters(1)
    log = m.get_current_log()
    assert list(log) == list(head["log"])
    for k, v in head["log"].items():
        print(f"{mode} aa{aa} {k}: {log[k]:.7f} record {v:.7f}")
        assert abs(log[k] - v) <= GATE * abs(v), k
    out = m.get_current_visuals()["result"]
    n, err, bound = _outside(out, head["output"])
    print(f"{mode} aa{aa} output: max err {err:.3e} bound {bound:.3e}")
    assert n == 0
    fake = ts.object_crops("fake")
    n, err, bound = _outside(fake, R.crop_resize_reference(ts.output().double().cpu(), mfx.boxes_of(head), bool(aa)), CROP_GATE)
    print(f"{mode} aa{aa} generated crops against the statement over the step's own output: max err {err:.3e} bound {bound:.3e}")
    assert n == 0
    assert _outside(fake, head["crops_gen"])[0] == 0
    g, d = _grads(ts)
    assert list(d) == [k for k, _ in head["d_keys"] if not k.endswith(("weight_u", "weight_v"))] and len(ts.d_state_dict()) == 50
    worst = ("", 0.0)
    for tag, ours, rec in (("G", g, head["g_grads"]), ("D", d, head["d_grads"])):
        assert list(ours) == list(rec)
        for k, ref in rec.items():
            if k.endswith("key_conv.bias"):
                assert float(ours[k].abs().max()) <= GATE * float(rec[k.replace(".bias", ".weight")].abs().max()), k
                continue
            n, err, bound = _outside(ours[k], ref)
            worst = max(worst, (f"{tag}.{k}", err / max(bound / GATE, 1e-300)), key=lambda t: t[1])
            assert n == 0, (tag, k, err, bound)
    print(f"{mode} aa{aa} worst gradient distance {worst[1]:.3e} of max|ref| ({worst[0]})")
    final_d = ts.d_state_dict()
    for ours, rec in ((ts.g_store.state_dict(), head["g_final"]), (final_d, head["d_final"]), (ts.ema_state_dict(), head["g_ema_final"])):
        for k, ref in rec.items():
            assert _outside(ours[k], ref)[0] == 0, k
    assert list(final_d) == [k for k, _ in head["d_keys"]]          # net_d's checkpoint: the reference's 50 keys in its order
    assert m.nonfinite_skips == {"net_g": 0, "net_d": 0}


def _step_cfg(head):
    from satlas_super_resolution_amd.train_step import StepConfig
    return StepConfig(l1_weight=head["l1_weight"], gan_weight=head["gan_weight"], lr_g=head["lr"], lr_d=head["lr"], betas=tuple(head["betas"]),
                      ema_decay=head["ema_decay"], feed_disc_lr=True, deterministic=True)


def _boxes_for_step(head, k):
    """different boxes for every step, n_osm_objs per image"""
    base = [[(0, 2, 3, 50, 40), (0, 20, 20, 52, 52)], [(0, 10, 5, 11, 30), (0, 0, 0, 64, 64)], [(0, 30, 31, 33, 64), (0, 1, 1, 9, 63)]][k]
    return [(b,) + q[1:] for b in range(2) for q in (base if b == 0 else base[::-1])]


def test_graph_equals_eager_bit_for_bit_with_new_boxes_every_step(heads):
    from satlas_super_resolution_amd.osm_train_step import OSMObjTrainStep
    head = heads[1]
    lr, hr = head["lr_u8"].float().cuda(), head["hr_u8"].float().cuda()
    runs = []
    for use_graph in (True, False):
        ts = OSMObjTrainStep(head["g_kwargs"], head["d_kwargs"], 2, 16, 16, "fp32", _step_cfg(head), n_osm_objs=2,
                             osm_obj_weight=head["osm_obj_weight"], antialias=True, use_graph=use_graph)
        ts.load_state(head["g0"], head["d0"])
        o_init = ts.o_store.data.clone()
        logs = []
        for k in range(3):               # graph: a warm-up pass, the capture, a replay
            ts.feed_data(lr.roll(k, 0), hr.roll(k, 0), scale=1.0 / 255)
            ts.set_boxes(_boxes_for_step(head, k))
            ts.step(k + 1)
            logs.append(ts.log())
        torch.cuda.synchronize()
        assert use_graph == ("step" in ts._graphs)
        runs.append((logs, ts.g_store.data.clone(), ts.d_store.data.clone(), ts.o_store.data.clone(), ts.opt_g.ema.clone()))
    (la, *a), (lb, *b) = runs
    assert la == lb and la[0] != la[1]
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(a[2], o_init)             # the object branch's arena was stepped


def test_save_and_resume_are_bit_identical(heads, tmp_path):
    head = heads[0]
    batches = [mfx.batch_of(head), dict(mfx.batch_of(head), lr=head["lr_u8"].flip(0), hr=head["hr_u8"].flip(0))]

    def feed(m, k):
        random.seed(100 + k)
        m.feed_data(batches[k])
        m.optimize_parameters(k + 1)

    a = _model(head, tmp_path, "fp32", deterministic=True)
    feed(a, 0)
    a.save(0, 1)
    feed(a, 1)
    opt = mfx.model_opt(head, tmp_path, "fp32", deterministic=True)
    opt["path"].update(pretrain_network_g=os.path.join(opt["path"]["models"], "net_g_1.pth"),
                       pretrain_network_d=os.path.join(opt["path"]["models"], "net_d_1.pth"))
    ck_d = torch.load(opt["path"]["pretrain_network_d"], weights_only=False)["params"]
    assert [(k, tuple(v.shape)) for k, v in ck_d.items()] == head["d_keys"]
    state = torch.load(os.path.join(opt["path"]["training_states"], "1.state"), weights_only=False)
    n_d = len([k for k, _ in head["d_keys"] if not k.endswith(("weight_u", "weight_v"))])
    sd = state["optimizers"][1]
    assert len(sd["state"]) == n_d == 34 and sd["param_groups"][0]["params"] == list(range(n_d))
    assert tuple(sd["state"][0]["exp_avg"].shape) == (64, 3, 4, 4) and tuple(sd["state"][n_d - 1]["exp_avg"].shape) == (1,)   # o_conv1.weight .. conv9.bias
    from satlas_super_resolution_amd.registry import MODEL_REGISTRY
    b = MODEL_REGISTRY.get("OSMObjESRGANModel")(opt)
    b.resume_training(state)
    random.seed(101)
    b.feed_data(batches[1])
    b.optimize_parameters(2)
    torch.cuda.synchronize()
    for x, y in ((a.ts.g_store.data, b.ts.g_store.data), (a.ts.d_store.data, b.ts.d_store.data), (a.ts.o_store.data, b.ts.o_store.data),
                 (a.ts.opt_g.ema, b.ts.opt_g.ema), (a.ts.opt_d.obj.exp_avg_sq, b.ts.opt_d.obj.exp_avg_sq),
                 (a.ts.opt_d.main.exp_avg, b.ts.opt_d.main.exp_avg)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(b.ts.opt_d.main.step) == int(b.ts.opt_d.obj.step) == 2


def test_one_guard_decision_for_both_arenas(heads):
    """a non-finite gradient in the object branch's arena alone keeps BOTH halves of the discriminator from stepping, counted once"""
    from satlas_super_resolution_amd.osm_train_step import OSMObjTrainStep
    head = heads[0]
    ts = OSMObjTrainStep(head["g_kwargs"], head["d_kwargs"], 2, 16, 16, "fp32", _step_cfg(head), n_osm_objs=2, use_graph=False)
    ts.load_state(head["g0"], head["d0"])
    before = (ts.d_store.data.clone(), ts.o_store.data.clone())
    ts.d_store.grad.fill_(1e-3)
    ts.o_store.grad.fill_(1e-3)
    ts.o_store.grad[5] = float("inf")
    ts.opt_d.update()
    torch.cuda.synchronize()
    assert torch.equal(ts.d_store.data, before[0]) and torch.equal(ts.o_store.data, before[1])
    assert ts.nonfinite_skips() == (0, 1) and int(ts.opt_d.main.step) == 0 and int(ts.opt_d.obj.step) == 0
    ts.o_store.grad[5] = 1e-3
    ts.opt_d.update()
    torch.cuda.synchronize()
    assert not torch.equal(ts.d_store.data, before[0]) and not torch.equal(ts.o_store.data, before[1])
    assert ts.nonfinite_skips() == (0, 1) and int(ts.opt_d.main.step) == 1 and int(ts.opt_d.obj.step) == 1


def test_refusals_by_name(heads, tmp_path):
    from satlas_super_resolution_amd.dp import DPContext
    from satlas_super_resolution_amd.osm_train_step import OSMObjTrainStep
    from satlas_super_resolution_amd.registry import MODEL_REGISTRY
    head = heads[0]
    with pytest.raises(NotImplementedError, match="bf16"):
        MODEL_REGISTRY.get("OSMObjESRGANModel")(mfx.model_opt(head, tmp_path, "bf16"))
    with pytest.raises(NotImplementedError, match="bf16"):
        OSMObjTrainStep(head["g_kwargs"], head["d_kwargs"], 2, 16, 16, "bf16", _step_cfg(head), n_osm_objs=2)
    with pytest.raises(NotImplementedError, match="world size 2"):
        OSMObjTrainStep(head["g_kwargs"], head["d_kwargs"], 2, 16, 16, "fp32", _step_cfg(head), n_osm_objs=2, dp=DPContext(None, 0, 2))
    with pytest.raises(NotImplementedError, match="world size 2"):
        MODEL_REGISTRY.get("OSMObjESRGANModel")(dict(mfx.model_opt(head, tmp_path), dist=True, world_size=2))
    m = _model(head, tmp_path)
    bad = dict(mfx.batch_of(head))
    m.osm_obj_data = dict(m.osm_obj_data, **{"7_11": {"building": [[70, 5, 90, 30], [1, 1, 9, 9]]}})
    with pytest.raises(ValueError, match="chip '7_11'"):          # an empty crop: on the host, naming the chip
        m.feed_data(bad)
    ts = m.ts
    with pytest.raises(ValueError, match="not a crop of image"):
        ts.set_boxes([(0, 0, 0, 65, 10), (0, 0, 0, 8, 8), (1, 0, 0, 8, 8), (1, 0, 0, 8, 8)])
    with pytest.raises(RuntimeError, match="no objects"):
        m.optimize_parameters(1)


def test_training_loop_on_the_miniature_dataset(heads, tmp_path):
    """satlas_super_resolution_amd.train.train end to end: S2NAIPDataset filtered by tests/golden/osm_mini (3 of the 5 chips keep two
    objects) -> DataLoader (collated `Chip` / `Phase`) -> OSMObjESRGANModel (128 x 128 images: boxes up to the full width, a fix-up
    box among them) -> logging, checkpoint, validation on the unfiltered split, whose batches carry no objects."""
    from conftest import GOLDEN
    from satlas_super_resolution_amd.train import train
    head = heads[0]
    mini = os.path.join(GOLDEN, "s2naip_mini")
    ds = {"name": "mini", "type": "S2NAIPDataset", "sentinel2_path": os.path.join(mini, "sentinel2"), "naip_path": os.path.join(mini, "naip"),
          "use_shuffle": False, "num_worker_per_gpu": 0, "batch_size_per_gpu": 2, "n_s2_images": 2}
    opt = mfx.model_opt(head, tmp_path, "fp32h")
    opt.update(name="mini", dist=False, datasets={"train": dict(ds, osm_objs_path=mfx.OSM_MINI, n_osm_objs=2), "val": dict(ds, name="validation")},
               val={"val_freq": 3, "save_img": False, "metrics": {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": False}}},
               logger={"print_freq": 1, "save_checkpoint_freq": 3})
    opt["path"]["visualization"] = str(tmp_path / "vis")
    opt["train"].update(total_iter=3, warmup_iter=-1, scheduler={"type": "MultiStepLR", "milestones": [400000], "gamma": 0.5})
    lines = []
    res = train(opt, log=lines.append)
    assert res["iters"] == 3 and res["epochs"] == 3          # one batch of two per epoch: three chips are left, the last is dropped
    assert list(res["log"]) == list(head["log"]) and all(v == v for v in res["log"].values())
    assert res["log"]["l_g_gan_objs"] > 0 and res["log"]["l_d_real"] > res["log"]["l_d_real_objs"] > 0
    assert 0 < res["metrics"]["psnr"] < 60
    ck = torch.load(tmp_path / "models" / "net_d_3.pth", weights_only=False)["params"]
    assert [(k, tuple(v.shape)) for k, v in ck.items()] == head["d_keys"]
