"""CPU: the host side of OSMObjESRGANModel - the tap rule of the crop resize against F.interpolate, the closed-form gradient of the
crops against autograd, the repair and slice resolution of the boxes, object sampling against the recorded run of the reference
(tools/make_osm_model_golden.py), the dataset filter, the registry name, the option function and the C ABI's argument checks.

Bounds: the tap rule is held to F.interpolate in float64 within 1e-12 (the two are the same formula in other association orders:
~1e-15 observed); the closed-form gradient to autograd within 1e-12 * max|gradient|; the float64 crops of the statement to the
float32 records of the reference within the float32 rounding of a convex combination, 1e-6 * max|record|."""
import json
import os
import random

import pytest
import torch
import torch.nn.functional as F

import osm_model_fixture as mfx
from conftest import GOLDEN

SIZES = (1, 2, 31, 32, 33, 64, 127, 128)


def _R():
    from satlas_super_resolution_amd import osm_reference
    return osm_reference


@pytest.fixture(scope="module")
def heads():
    return [mfx.load(0), mfx.load(1)]


@pytest.mark.parametrize("antialias", (False, True))
def test_tap_rule_equals_interpolate_in_float64(antialias):
    R = _R()
    g = torch.Generator().manual_seed(7)
    worst, taps = 0.0, 0
    for h in SIZES:
        for w in SIZES:
            x = torch.randn(1, 3, h, w, dtype=torch.float64, generator=g)
            ref = F.interpolate(x, size=(32, 32), mode="bilinear", align_corners=False, antialias=antialias)
            out = R.crop_resize_reference(x, [(0, 0, 0, w, h)], antialias)
            worst = max(worst, float((out - ref).abs().max()))
        taps = max(taps, max(c for _, c, _ in R.resize_taps(h, 32, antialias)))
    assert worst <= 1e-12, worst
    assert taps <= (8 if antialias else 2)          # what csrc/obj_crop.hip sizes its tap tables for


def test_identity_size_has_unit_weights():
    for aa in (False, True):
        m = _R().resize_matrix(32, 32, aa)
        assert torch.equal(m, torch.eye(32, dtype=torch.float64))


@pytest.mark.parametrize("antialias", (False, True))
def test_closed_form_crop_gradient_equals_autograd(antialias):
    R = _R()
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 3, 40, 48, dtype=torch.float64, generator=g).requires_grad_(True)
    boxes = [(0, 5, 7, 6, 8), (0, 0, 0, 48, 40), (0, 3, 4, 36, 35), (1, 5, 5, 25, 20), (1, 15, 10, 39, 33)]
    w = torch.randn(len(boxes), 3, 32, 32, dtype=torch.float64, generator=g)
    (R.crop_resize_reference(img, boxes, antialias) * w).sum().backward()
    closed = R.crop_resize_backward(w, boxes, img.shape, antialias)
    assert float((closed - img.grad).abs().max()) <= 1e-12 * float(img.grad.abs().max())


def test_fix_up_and_slice_resolution():
    R = _R()
    assert R.fix_box([10, 5, 10, 30]) == (10, 5, 11, 30)                 # x1 == x2 below 128: widened to the right
    assert R.fix_box([128, 5, 128, 30]) == (127, 5, 128, 30)             # x2 = 128: the second branch, widened to the left
    assert R.fix_box([3, 128, 9, 128]) == (3, 127, 9, 128)
    assert R.fix_box([3, 200, 9, 200]) == (3, 199, 9, 200)               # the literal 128 whatever the image size
    assert R.fix_box([1, 2, 3, 4]) == (1, 2, 3, 4)
    # Python slice semantics: negative indices count from the end, over-long ones stop at the edge
    assert R.resolve_boxes([[-20, 4, -4, 30]], 64, 64, "c") == [(44, 4, 60, 30)]
    assert R.resolve_boxes([[50, 10, 300, 90]], 64, 64, "c") == [(50, 10, 64, 64)]
    assert R.resolve_boxes([[128, 5, 128, 30]], 128, 128, "c") == [(127, 5, 128, 30)]
    for box in ([70, 5, 90, 30], [30, 5, 20, 30], [64, 0, 64, 10]):      # beyond the image, reversed, a fix-up that lands outside
        with pytest.raises(ValueError, match="chip '12_34'"):
            R.resolve_boxes([[1, 1, 5, 5], box], 64, 64, "12_34")


def test_sample_objects_reproduces_the_recorded_run(heads):
    R = _R()
    for head in heads:
        random.seed(head["seed"])
        chosen = [R.sample_objects(head["chips"][c], head["n_osm_objs"], random) for c in head["chip_names"]]
        assert chosen == head["chosen"]
        assert random.random() == head["random_after"]       # the stream is where the reference leaves it
        assert all(idx == sorted(idx) for idx in chosen)
    assert heads[0]["chosen"] != heads[1]["chosen"]
    with pytest.raises(ValueError):                              # random.sample's own: fewer objects than n_osm_objs
        R.sample_objects({"building": [[1, 2, 3, 4]]}, 2, random)
    rng = random.Random(5)                                        # any generator with random's interface
    assert len(R.sample_objects(heads[0]["chips"]["7_12"], 3, rng)) == 3


def test_statement_crops_equal_the_recorded_crops(heads):
    """the reference's own crops of the real image (its resize stand-in is F.interpolate, float32) against the float64 statement over
    the boxes the project's host code resolves: the fix-up box, the downscaled box and the overlapping pair are among them"""
    R = _R()
    sides = set()
    for head in heads:
        boxes = mfx.boxes_of(head)
        sides |= {(x2 - x1, y2 - y1) for _, x1, y1, x2, y2 in boxes}
        gt = (head["hr_u8"].float() / 255).double()
        out = R.crop_resize_reference(gt, boxes, head["antialias"])
        rec = head["crops_gt"].double()
        assert float((out - rec).abs().max()) <= 1e-6 * float(rec.abs().max())
    assert (1, 25) in sides and (48, 37) in sides and (32, 32) in sides


def test_fixture_conditions(heads):
    for head in heads:
        gated = {k: v for k, v in head["f32_to_f64"].items() if not k.endswith("key_conv.bias")}
        assert max(gated.values()) <= 1e-4, max(gated.items(), key=lambda kv: kv[1])
        assert list(head["log"]) == ["l_g_pix", "l_g_gan", "l_g_gan_objs", "l_d_real", "l_d_real_objs", "out_d_real", "l_d_fake",
                                     "l_d_fake_objs", "out_d_fake"]
        assert len(head["d_keys"]) == 50 and head["d_keys"][:len(mfx.fx.OBJ_KEYS)] == mfx.fx.OBJ_KEYS
        assert float(head["d_grads"]["o_conv1.weight"].abs().max()) > 0 and head["log"]["l_g_gan_objs"] > 0
    for f in os.listdir(GOLDEN):
        if f.startswith("osm_model_"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 1 << 20, f


def _dataset_opt(**over):
    mini = os.path.join(GOLDEN, "s2naip_mini")
    opt = dict(phase="train", name="train", n_s2_images=2, scale=4, sentinel2_path=os.path.join(mini, "sentinel2"),
               naip_path=os.path.join(mini, "naip"))
    opt.update(over)
    return opt


def test_dataset_filter_on_osm_mini():
    from satlas_super_resolution_amd.data.s2naip_dataset import S2NAIPDataset
    chips = lambda ds: [dp[2] for dp in ds.datapoints]
    every = chips(S2NAIPDataset(_dataset_opt()))
    assert sorted(every) == ["100_200", "100_201", "101_200", "101_201", "102_200"]
    kept = chips(S2NAIPDataset(_dataset_opt(osm_objs_path=mfx.OSM_MINI, n_osm_objs=2)))
    assert kept == [c for c in every if c in ("100_200", "101_200", "101_201")]          # the rule, and the order unchanged
    assert chips(S2NAIPDataset(_dataset_opt(osm_objs_path=mfx.OSM_MINI, n_osm_objs=1))) == [c for c in every if c != "102_200"]
    assert chips(S2NAIPDataset(_dataset_opt(osm_objs_path=mfx.OSM_MINI, n_osm_objs=4))) == []
    assert chips(S2NAIPDataset(_dataset_opt(phase="val", osm_objs_path=mfx.OSM_MINI, n_osm_objs=2))) == every    # other splits ignore it
    ds = S2NAIPDataset(_dataset_opt(osm_objs_path=mfx.OSM_MINI, n_osm_objs=2))
    random.seed(0)
    s = ds[0]
    assert s["Chip"] in kept and s["Phase"] == "train"          # (a sample the loader skips moves on to the next kept chip)


def test_registry_and_option_function():
    import satlas_super_resolution_amd.models  # noqa: F401  (discovers every *_model.py, as the training loop's import does)
    from satlas_super_resolution_amd.registry import MODEL_REGISTRY
    cls = MODEL_REGISTRY.get("OSMObjESRGANModel")
    from satlas_super_resolution_amd.models import osm_objs_esrgan_model as M
    from satlas_super_resolution_amd.models.ssr_esrgan_model import SSRESRGANModel
    assert cls is M.OSMObjESRGANModel and issubclass(cls, SSRESRGANModel)
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["osm_obj_esrgan.yml"]
    c = M.osm_config_from_opt(opt)
    assert c.osm_obj_weight == 0.3 and c.n_osm_objs == 1 and c.antialias is False
    assert c.osm_objs_path == opt["datasets"]["train"]["osm_objs_path"]
    assert c.step.feed_disc_lr and c.step.gan_weight == opt["train"]["gan_opt"]["loss_weight"]
    assert M.osm_config_from_opt(dict(opt, osm_obj_resize_antialias=True)).antialias is True


def test_refusals_by_name(monkeypatch):
    from satlas_super_resolution_amd.models import osm_objs_esrgan_model as M
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["osm_obj_esrgan.yml"]
    for k in ("clip_opt", "ldl_opt"):
        with pytest.raises(NotImplementedError, match=k):
            M.osm_config_from_opt(dict(opt, train=dict(opt["train"], **{k: {"type": "X", "loss_weight": 1.0}})))
    with pytest.raises(NotImplementedError, match="bf16"):
        M.osm_config_from_opt(dict(opt, compute_dtype="bf16"))
    with pytest.raises(NotImplementedError, match="OSMObjDiscriminator"):
        M.osm_config_from_opt(dict(opt, network_d=dict(opt["network_d"], type="SSR_UNetDiscriminatorSN")))
    with pytest.raises(NotImplementedError, match="world size 2"):
        M.osm_config_from_opt(dict(opt, dist=True, world_size=2))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="world size 2"):
        M.osm_config_from_opt(opt)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(KeyError, match="osm_obj_weight"):
        M.osm_config_from_opt({k: v for k, v in opt.items() if k != "osm_obj_weight"})
    # the existing option functions keep their refusals: the model type is not theirs to accept
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt
    with pytest.raises(NotImplementedError, match="clip_opt"):
        step_config_from_opt(dict(opt, train=dict(opt["train"], clip_opt={"type": "X"})))


def test_crop_entries_are_exported_and_reject_bad_arguments_without_a_launch():
    from satlas_super_resolution_amd import build, hip
    L = hip.lib()
    for s in ("ssr_obj_crop_resize_fwd", "ssr_obj_crop_resize_bwd"):
        assert s in hip.ABI_SYMBOLS and hasattr(L, s)
    assert "obj_crop.hip" in build.SOURCES and L.ssr_abi_version() == 3
    assert hip.OBJ_CROP == 32 and hip.OBJ_MAX_SIDE >= 128
    fake = 1 << 20                      # a 16-byte aligned address that is never dereferenced: every call below fails its checks first
    img, crop = hip.View(fake, 8, 0), hip.View(fake, 8, 0)

    def fwd(src=img, dtype=hip.F32, B=2, H=40, W=40, boxes=fake, Bo=3, dst=crop):
        return L.ssr_obj_crop_resize_fwd(src, dtype, B, H, W, boxes, Bo, dst, 0, None)

    def bwd(g=crop, boxes=fake, first=fake, Bo=3, dimg=hip.View(fake + 4096, 8, 0), dtype=hip.F32, B=2, H=40, W=40):
        return L.ssr_obj_crop_resize_bwd(g, boxes, first, Bo, dimg, dtype, B, H, W, 1.0, 0, None)

    for over in (dict(B=0), dict(H=0), dict(W=-1), dict(Bo=0), dict(boxes=None), dict(boxes=fake + 2), dict(src=hip.View(None, 8, 0)),
                 dict(src=hip.View(fake + 2, 8, 0)), dict(src=hip.View(fake, 8, 6)), dict(src=hip.View(fake, 2, 0)), dict(dst=hip.View(None, 8, 0)),
                 dict(dst=hip.View(fake + 4, 8, 0)), dict(dst=hip.View(fake, 6, 0)), dict(dst=hip.View(fake, 12, 8)), dict(dst=hip.View(fake, 16, 2)),
                 dict(dtype=7), dict(dtype=hip.F32H3)):
        assert fwd(**over) == -1, over
    for over in (dict(B=0), dict(Bo=0), dict(boxes=None), dict(first=None), dict(first=fake + 1), dict(g=hip.View(None, 8, 0)),
                 dict(g=hip.View(fake, 4, 0)), dict(dimg=hip.View(None, 8, 0)), dict(dimg=hip.View(fake + 4096, 8, 6)), dict(dimg=crop), dict(dtype=9)):
        assert bwd(**over) == -1, over
    # bf16 storage: unsupported, as the object branch itself; still without a launch
    assert fwd(dtype=hip.BF16) == -2 and bwd(dtype=hip.BF16) == -2
    assert bwd(B=70000) == -2
