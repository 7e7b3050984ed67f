"""CPU: the CLIP loss of train.clip_opt - option parsing and its refusals, the golden fixture against the project's own float64
statements (autograd and the closed-form gradient), the inverse of the nearest-resize index table, and the C ABI of csrc/vit_bwd.hip
as far as it can be exercised without a device (exports, refusals that launch nothing)."""
import copy
import ctypes as C
import json
import os

import pytest
import torch

import cliploss_fixture as LF
from conftest import GOLDEN

SHIPPED = "cliploss_esrgan_s2naip_urban.yml"


def _opts():
    return json.load(open(os.path.join(GOLDEN, "ssr_options.json")))


@pytest.fixture()
def weights(tmp_path):
    path = str(tmp_path / "tower_a.pth")
    torch.save(LF.tower_state("A"), path)
    return path


def _with(opt, **clip):
    o = copy.deepcopy(opt)
    o["train"]["clip_opt"].update(clip)
    return o


# ------------------------------------------------------------------ options
def test_shipped_file_parses_with_weights_and_equals_the_urban_file_apart_from_clip(weights, monkeypatch):
    from satlas_super_resolution_amd.models.ssr_esrgan_model import step_config_from_opt, train_config_from_opt
    from satlas_super_resolution_amd.train_step import N_LOSS, StepConfig
    monkeypatch.delenv("SSR_CLIP_LOSS_SIGLIP_B16_WEIGHTS", raising=False)
    opts = _opts()
    opt = _with(opts[SHIPPED], clip_weights=weights)
    before = copy.deepcopy(opt)
    cfg = train_config_from_opt(opt)
    assert opt == before                                              # the caller's dictionary is left as it was
    assert cfg.clip == {"model": "ViT-B-16-SigLIP-256", "family": "siglip", "path": os.path.abspath(weights), "gelu": "tanh", "loss_weight": 1.0}
    urban = step_config_from_opt(opts["esrgan_s2naip_urban.yml"])
    assert urban.clip is None and StepConfig().clip is None
    urban.clip = cfg.clip
    assert cfg == urban
    assert train_config_from_opt(_with(opt, loss_weight=0.25, gelu="erf")).clip["loss_weight"] == 0.25
    assert train_config_from_opt(_with(opt, gelu="erf")).clip["gelu"] == "erf"
    with pytest.raises(NotImplementedError, match="clip_opt"):        # the older function still refuses (tests/test_host_boundary.py)
        step_config_from_opt(opt)
    assert N_LOSS == 9                                                # l_clip_sim has a buffer of its own


def test_weights_are_found_in_three_places_and_their_absence_is_named(weights, monkeypatch, tmp_path):
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    opt = _opts()[SHIPPED]
    monkeypatch.delenv(CL.CLIP_LOSS_ENV, raising=False)
    monkeypatch.chdir(tmp_path)                                       # no experiments/pretrained_models here
    with pytest.raises(NotImplementedError, match=r"^train\.clip_opt:") as e:
        train_config_from_opt(opt)
    msg = str(e.value)
    assert "clip_weights" in msg and CL.CLIP_LOSS_ENV in msg and CL.CLIP_LOSS_PRETRAIN_PATH in msg and "torch.save(open_clip" in msg
    assert ".visual.state_dict()" in msg
    monkeypatch.setenv(CL.CLIP_LOSS_ENV, weights)
    assert train_config_from_opt(opt).clip["path"] == os.path.abspath(weights)
    monkeypatch.delenv(CL.CLIP_LOSS_ENV)
    os.makedirs(os.path.dirname(CL.CLIP_LOSS_PRETRAIN_PATH))
    torch.save(LF.tower_state("A"), CL.CLIP_LOSS_PRETRAIN_PATH)
    assert train_config_from_opt(opt).clip["path"] == os.path.abspath(CL.CLIP_LOSS_PRETRAIN_PATH)
    monkeypatch.setenv(CL.CLIP_LOSS_ENV, str(tmp_path / "nowhere.pth"))      # the option comes first, then the variable, then the default
    assert train_config_from_opt(_with(opt, clip_weights=weights)).clip["path"] == os.path.abspath(weights)
    with pytest.raises(FileNotFoundError, match="clip_opt"):
        train_config_from_opt(_with(opt, clip_weights=str(tmp_path / "missing.pth")))


def test_refusals_by_name(weights, monkeypatch):
    from satlas_super_resolution_amd.models import osm_objs_esrgan_model as OM
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    opts = _opts()
    opt = _with(opts[SHIPPED], clip_weights=weights)
    for name, why in (("EVA02-E-14-plus", "4.4 B"), ("RN50", "ResNet")):
        with pytest.raises(NotImplementedError, match=rf"clip_opt\.clip_loss_model='{name}'.*{why}"):
            train_config_from_opt(_with(opt, clip_loss_model=name))
    with pytest.raises(NotImplementedError, match=r"clip_opt\.clip_loss_model='ViT-L-14'"):
        train_config_from_opt(_with(opt, clip_loss_model="ViT-L-14"))
    with pytest.raises(NotImplementedError, match=r"clip_opt\.type='Other'"):
        train_config_from_opt(_with(opt, type="Other"))
    with pytest.raises(NotImplementedError, match=r"clip_opt\.reduction"):
        train_config_from_opt(_with(opt, reduction="sum"))
    with pytest.raises(NotImplementedError, match=r"clip_opt\.gelu='relu'"):
        train_config_from_opt(_with(opt, gelu="relu"))
    with pytest.raises(NotImplementedError, match=r"clip_opt.*bf16"):
        train_config_from_opt(dict(opt, compute_dtype="bf16"))
    with pytest.raises(NotImplementedError, match=r"clip_opt.*bf16"):
        train_config_from_opt(dict(opt, network_g=dict(opt["network_g"], compute_dtype="bf16")))
    with pytest.raises(NotImplementedError, match=r"clip_opt.*world size 2"):
        train_config_from_opt(dict(opt, dist=True, world_size=2))
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(NotImplementedError, match=r"clip_opt.*world size 4"):
        train_config_from_opt(opt)
    monkeypatch.delenv("WORLD_SIZE")
    # OSMObjESRGANModel keeps refusing the block, valid or not
    osm = opts["osm_obj_esrgan.yml"]
    with pytest.raises(NotImplementedError, match=r"clip_opt.*OSMObjESRGANModel"):
        OM.osm_config_from_opt(dict(osm, train=dict(osm["train"], clip_opt=opt["train"]["clip_opt"])))


def test_clip_family_has_no_backward():
    import clipscore_fixture as FX
    from satlas_super_resolution_amd import clip_loss as CL
    x = torch.rand(1, 3, 8, 8, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="clip_opt.*class token"):
        CL.clip_loss_grad_reference(x, x, FX.tiny_state("clip"))


# ------------------------------------------------------------------ the golden fixture
@pytest.fixture(scope="module")
def golden():
    return LF.load_golden()


CASES = [(t, h, w) for t in LF.TOWERS for h, w in LF.SIZES]


def test_golden_file_holds_inputs_and_results_only(golden):
    assert set(golden["cases"]) == {LF.case_key(*c) for c in CASES} and golden["loss_weight"] == LF.LOSS_WEIGHT
    assert golden["towers"] == LF.TOWERS and golden["tower_seed"] == LF.TOWER_SEED
    for c in golden["cases"].values():
        assert set(c) == {"seed", "fake_u8", "gt_u8", "loss", "grad", "margin"}
        assert c["fake_u8"].dtype == torch.uint8 and c["grad"].dtype == torch.float64 and c["grad"].shape == c["fake_u8"].shape
    assert os.path.getsize(LF.PATH) < 1 << 20


@pytest.mark.parametrize("case", CASES, ids=[LF.case_key(*c) for c in CASES])
def test_golden_matches_both_float64_statements(golden, case):
    """the package's loss and autograd gradient against clip_loss_reference under autograd and against clip_loss_grad_reference
    (closed form), both to 1e-9 of max|ref|; and the sign margin, recomputed here from the project's own features"""
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd.clipscore_metric import vit_config_from_state, vit_features_from_input
    tower, h, w = case
    c = golden["cases"][LF.case_key(tower, h, w)]
    fake_u8, gt_u8 = LF.images(c["seed"], h, w)                      # the images are the fixture rule's
    assert torch.equal(fake_u8, c["fake_u8"]) and torch.equal(gt_u8, c["gt_u8"])
    fake, gt, sd = LF.to_float(fake_u8).double(), LF.to_float(gt_u8).double(), LF.tower_state(tower)
    ref_l, ref_g = float(c["loss"]), c["grad"]
    f = fake.clone().requires_grad_(True)
    loss = CL.clip_loss_reference(f, gt, sd, LF.LOSS_WEIGHT, "tanh", torch.float64)
    loss.backward()
    assert abs(float(loss.detach()) - ref_l) <= 1e-9 * abs(ref_l)
    assert float((f.grad - ref_g).abs().max()) <= 1e-9 * float(ref_g.abs().max())
    l2, g2 = CL.clip_loss_grad_reference(fake, gt, sd, LF.LOSS_WEIGHT, "tanh", torch.float64)
    assert abs(float(l2) - ref_l) <= 1e-9 * abs(ref_l)
    assert float((g2 - ref_g).abs().max()) <= 1e-9 * float(ref_g.abs().max())
    size = vit_config_from_state(sd)["image_size"]
    with torch.no_grad():
        fx, fg = (vit_features_from_input(CL.clip_loss_input(t, size, torch.float64), sd, "tanh") for t in (fake, gt))
    margin = float((fx - fg).abs().min() / fx.abs().max())
    assert margin >= LF.SIGN_MARGIN and abs(margin - c["margin"]) <= 1e-9


def test_closed_form_gradient_with_the_erf_activation():
    from satlas_super_resolution_amd import clip_loss as CL
    sd = LF.tower_state("B")
    fake, gt = (LF.to_float(t).double() for t in LF.images(0, 20, 24))
    f = fake.clone().requires_grad_(True)
    CL.clip_loss_reference(f, gt, sd, 1.0, "erf").backward()
    _, g = CL.clip_loss_grad_reference(fake, gt, sd, 1.0, "erf")
    assert float((g - f.grad).abs().max()) <= 1e-12 * float(f.grad.abs().max())


def test_clip_loss_input_is_the_nearest_resize_then_openai_mean_std():
    import torch.nn.functional as F
    from satlas_super_resolution_amd import clip_loss as CL
    x = torch.rand(2, 3, 50, 40, dtype=torch.float64)
    mean = torch.tensor((0.48145466, 0.4578275, 0.40821073), dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711), dtype=torch.float32).double().view(1, 3, 1, 1)
    want = (F.interpolate(x, (144, 144)) - mean) / std
    assert torch.equal(CL.clip_loss_input(x, 144, torch.float64), want)


# ------------------------------------------------------------------ nearest_inverse_ranges
@pytest.mark.parametrize("n_in,n_out,used", [(5, 48, None), (36, 144, None), (50, 144, None), (48, 48, None), (100, 48, None), (50, 144, 100),
                                             (100, 48, 40), (7, 48, 0)])
def test_nearest_inverse_ranges_inverts_the_index_table(n_in, n_out, used):
    from satlas_super_resolution_amd.clip_loss import nearest_inverse_ranges
    from satlas_super_resolution_amd.clipscore_metric import nearest_index_table
    table = nearest_index_table(n_in, n_out)
    r = nearest_inverse_ranges(n_in, n_out, used)
    lim = n_out if used is None else used
    assert r.shape == (n_in, 2) and r.dtype == torch.int64
    seen = torch.zeros(lim, dtype=torch.int64)
    for i in range(n_in):
        lo, hi = int(r[i, 0]), int(r[i, 1])
        assert 0 <= lo <= hi <= lim
        assert bool((table[lo:hi] == i).all())                       # every destination in the range reads source i
        seen[lo:hi] += 1
    assert bool((seen == 1).all())                                    # and every destination below `used` is in exactly one range
    if n_in > n_out:
        assert int((r[:, 1] == r[:, 0]).sum()) >= n_in - n_out       # sources that nothing reads: empty ranges


# ------------------------------------------------------------------ the C ABI, as far as a machine without a GPU can see it
NEW_ENTRIES = ("ssr_vit_float_input", "ssr_vit_float_input_bwd", "ssr_layernorm_bwd", "ssr_vit_act_fwd", "ssr_vit_act_bwd", "ssr_mha_bwd",
               "ssr_mha_bwd_ws_floats", "ssr_feature_l1")


def test_entries_are_exported_and_reject_bad_arguments_without_a_launch():
    """every refusal below is decided on the host before any device call, so it returns its code on a machine without a GPU"""
    from satlas_super_resolution_amd import build, hip
    L = hip.lib()
    for s in NEW_ENTRIES:
        assert s in hip.ABI_SYMBOLS and hasattr(L, s)
    assert "vit_bwd.hip" in build.SOURCES and L.ssr_abi_version() == 3
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)
    p += (-p) % 16
    v, NV = hip.View(p, 128, 0), hip.NULL_VIEW
    assert L.ssr_layernorm_bwd(v, p, v, NV, v, hip.BF16, 4, 128, 1e-6, None) == -2
    assert L.ssr_layernorm_bwd(v, p, v, NV, v, hip.F32, 4, 126, 1e-6, None) == -2
    assert L.ssr_layernorm_bwd(v, None, v, NV, v, hip.F32, 4, 128, 1e-6, None) == -1
    assert L.ssr_layernorm_bwd(v, p, v, NV, NV, hip.F32, 4, 128, 1e-6, None) == -1
    assert L.ssr_layernorm_bwd(v, p, v, hip.View(p + 4, 128, 0), v, hip.F32, 4, 128, 1e-6, None) == -1      # a misaligned residual
    assert L.ssr_vit_act_fwd(v, v, hip.F32, 4, 128, 7, None) == -1 and L.ssr_vit_act_fwd(v, v, hip.BF16, 4, 128, 2, None) == -2
    assert L.ssr_vit_act_bwd(v, NV, v, hip.F32, 4, 128, 2, None) == -1 and L.ssr_vit_act_bwd(v, v, v, hip.F32, 4, 130, 2, None) == -2
    assert L.ssr_mha_bwd(v, v, v, v, NV, v, v, p, hip.F32, 1, 4, 4, 2, 32, 0.1, None) == -2                  # head dims 64 and 72 only
    assert L.ssr_mha_bwd(v, v, v, v, NV, v, v, None, hip.F32, 1, 4, 4, 2, 64, 0.1, None) == -1              # no workspace
    assert L.ssr_mha_bwd(v, v, v, v, NV, NV, v, p, hip.F32, 1, 4, 4, 2, 64, 0.1, None) == -1                # dk is not optional
    assert L.ssr_mha_bwd(v, v, v, v, NV, v, v, p, hip.F32, 1, 4, 4, 3, 64, 0.1, None) == -1                 # 3 x 64 channels in a 128-wide view
    assert L.ssr_mha_bwd(v, v, v, v, NV, v, v, p, hip.F32, 1, 0, 4, 2, 64, 0.1, None) == -1
    assert L.ssr_mha_bwd_ws_floats(2, 81, 2) == 3 * 2 * 81 * 2 and L.ssr_mha_bwd_ws_floats(0, 1, 1) == -1
    assert L.ssr_feature_l1(v, v, v, 4, 128, 1.0, None, 0, None) == -1 and L.ssr_feature_l1(v, v, v, 4, 128, 1.0, p, 5, None) == -1
    assert L.ssr_feature_l1(v, v, v, 4, 129, 1.0, p, 0, None) == -1
    perm, twice = (C.c_int32 * 3)(0, 1, 2), (C.c_int32 * 3)(1, 1, 2)
    std = (C.c_float * 3)(1.0, 0.0, 1.0)
    img = hip.View(p, 8, 0)
    assert L.ssr_vit_float_input(img, 1, 4, 4, p, p, 1, 2, v, hip.F32, twice, None, None, None) == -1        # not a permutation
    assert L.ssr_vit_float_input(img, 1, 4, 4, p, p, 1, 66, v, hip.F32, perm, None, None, None) == -2
    assert L.ssr_vit_float_input(img, 1, 4, 4, None, p, 1, 2, v, hip.F32, perm, None, None, None) == -1
    assert L.ssr_vit_float_input(hip.View(p, 8, 6), 1, 4, 4, p, p, 1, 2, v, hip.F32, perm, None, None, None) == -1   # channels 6 .. 8 of 8
    assert L.ssr_vit_float_input_bwd(v, 1, 4, 4, p, p, 1, 2, img, hip.F32, perm, std, None) == -1           # a zero std
    assert L.ssr_vit_float_input_bwd(v, 1, 4, 4, p, p, 1, 2, img, hip.BF16, perm, None, None) == -2
    assert all(x == 0.0 for x in buf)
