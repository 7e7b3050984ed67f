"""Host: the arithmetic model of `tower_arithmetic: split` (satlas_super_resolution_amd/linear_split.py) and its options.

  * linear_split_reference against the float64 product within split_representation_bound, for both piece encodings, over the shapes
    of tests/test_gpu_linear_split.py and value regimes that reach fp16's subnormals (x 2^-16, 2^-10, 1e-7; w 2^-12), its top (x 7.5e3,
    w 30) and ordinary values;
  * the closed-form loss and image gradient with every product replaced by the model (fp16 pieces forward, bf16 pieces in the
    transposes) against the golden cases of tests/golden/cliploss_siglip_tiny.pt at the gates of tests/test_gpu_clip_loss.py;
  * the option's values in train.clip_opt and in calculate_clipscore, and the |w| >= 64 refusal by matrix name.
"""
import functools

import pytest
import torch

import cliploss_fixture as LF
import clipscore_fixture as FX

SHAPES = [(1, 4, 4), (5, 20, 12), (33, 200, 68), (130, 588, 132), (64, 768, 256)]
X_REGIMES = {"1": 1.0, "2^-16": 2.0 ** -16, "2^-10": 2.0 ** -10, "7.5e3": 7.5e3, "1e-7": 1e-7}
W_REGIMES = {"1": 1.0, "30": 30.0, "2^-12": 2.0 ** -12}


def _operands(M, K, Nout, xs, ws):
    """x normal with standard deviation xs (|x| <= 5.5 xs < 65504 for xs = 7.5e3); w uniform in (-ws, ws): inside |w| < 64"""
    g = torch.Generator().manual_seed(M * 7919 + K * 31 + Nout)
    x = (torch.randn(M, K, generator=g) * xs).clamp(-5.5 * xs, 5.5 * xs)
    w = (2 * torch.rand(Nout, K, generator=g) - 1) * ws
    return x, w


@pytest.mark.parametrize("pieces", ["f16", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_piece_model_is_within_the_representation_bound(shape, pieces):
    from satlas_super_resolution_amd import linear_split as S
    worst = 0.0
    for xn, xs in X_REGIMES.items():
        for wn, ws in W_REGIMES.items():
            x, w = _operands(*shape, xs, ws)
            truth = x.double() @ w.double().t()
            err = (S.linear_split_reference(x, w, None, pieces) - truth).abs()
            bound = S.split_representation_bound(x, w, pieces)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert bool((err <= bound).all()), (xn, wn, ratio)
    print(f"linear_split_reference {shape} {pieces}: worst |err| / bound over the regimes {worst:.3f}")


def test_piece_model_adds_the_bias_and_keeps_leading_axes():
    from satlas_super_resolution_amd import linear_split as S
    x, w = _operands(6, 20, 12, 1.0, 1.0)
    b = torch.linspace(-1, 1, 12)
    y = S.linear_split_reference(x.reshape(2, 3, 20), w, b, "f16")
    assert y.shape == (2, 3, 12) and y.dtype == torch.float64
    assert torch.equal(y.reshape(6, 12), S.linear_split_reference(x, w, None, "f16") + b.double())
    # an operand that 11 bits hold is its own hi piece: the product is exact
    xe, we = torch.tensor([[1.5, -2.0, 0.25, 3.0]]), torch.tensor([[0.5, 1.0, -4.0, 2.0]])
    for pieces in ("f16", "bf16"):
        assert float(S.linear_split_reference(xe, we, None, pieces)) == float(xe.double() @ we.double().t())


@functools.lru_cache(maxsize=None)
def _golden():
    return LF.load_golden()


@pytest.mark.parametrize("case", [(t, h, w) for t in LF.TOWERS for h, w in LF.SIZES], ids=lambda c: LF.case_key(*c))
def test_split_closed_form_meets_the_gates_of_the_device_test(case):
    from satlas_super_resolution_amd import clip_loss as CL
    tower, h, w = case
    c = _golden()["cases"][LF.case_key(tower, h, w)]
    assert c["margin"] >= LF.SIGN_MARGIN
    fake, gt = LF.to_float(c["fake_u8"]), LF.to_float(c["gt_u8"])
    loss, grad = CL.clip_loss_grad_reference(fake, gt, LF.tower_state(tower), LF.LOSS_WEIGHT, "tanh", torch.float64, tower_arithmetic="split")
    el = abs(float(loss) - float(c["loss"])) / float(c["loss"])
    ref = float(c["grad"].abs().max())
    delta = (grad - c["grad"]).abs()
    outside = int((delta > 1e-3 * ref).sum())
    print(f"split closed form {tower} {h}x{w}: loss |err| / ref {el:.3e}, gradient max |delta| / max|ref| {float(delta.max()) / ref:.3e}, "
          f"{outside} outside 1e-3")
    assert el <= 1e-4
    assert outside == 0
    # the model is not the exact path: the two differ, by less than the gate
    loss_e, grad_e = CL.clip_loss_grad_reference(fake, gt, LF.tower_state(tower), LF.LOSS_WEIGHT, "tanh", torch.float64)
    assert not torch.equal(grad, grad_e) and float((grad - grad_e).abs().max()) <= 1e-3 * ref


def test_closed_form_refuses_an_unknown_arithmetic():
    from satlas_super_resolution_amd import clip_loss as CL
    c = _golden()["cases"][LF.case_key("B", *LF.SIZES[0])]
    fake, gt = LF.to_float(c["fake_u8"]), LF.to_float(c["gt_u8"])
    with pytest.raises(NotImplementedError, match="tower_arithmetic='fp16'"):
        CL.clip_loss_grad_reference(fake, gt, LF.tower_state("B"), tower_arithmetic="fp16")


def test_clip_opt_takes_exact_and_split_and_refuses_the_rest(tmp_path):
    from satlas_super_resolution_amd import clip_loss as CL
    wfile = tmp_path / "w.pth"
    wfile.write_bytes(b"")
    base = {"type": "CLIPLoss", "clip_loss_model": "ViT-B-16-SigLIP-256", "clip_weights": str(wfile)}
    assert "tower_arithmetic" in CL._CLIP_OPT_KEYS
    absent = CL.check_clip_opt(dict(base))
    assert CL.check_clip_opt(dict(base, tower_arithmetic="exact")) == absent and "tower_arithmetic" not in absent
    assert CL.check_clip_opt(dict(base, tower_arithmetic="split")) == dict(absent, tower_arithmetic="split")
    for bad in ("fp16", "Split", "", 1):
        with pytest.raises(NotImplementedError) as e:
            CL.check_clip_opt(dict(base, tower_arithmetic=bad))
        assert str(e.value).startswith(f"train.clip_opt.tower_arithmetic={bad!r}")


def test_clip_opt_reaches_the_step_config(tmp_path):
    import json
    import os

    from conftest import GOLDEN
    from satlas_super_resolution_amd.models.ssr_esrgan_model import train_config_from_opt
    wfile = tmp_path / "w.pth"
    wfile.write_bytes(b"")
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["cliploss_esrgan_s2naip_urban.yml"]
    opt["train"]["clip_opt"]["clip_weights"] = str(wfile)
    assert "tower_arithmetic" not in train_config_from_opt(json.loads(json.dumps(opt))).clip
    opt["train"]["clip_opt"]["tower_arithmetic"] = "split"
    assert train_config_from_opt(json.loads(json.dumps(opt))).clip["tower_arithmetic"] == "split"
    opt["train"]["clip_opt"]["tower_arithmetic"] = "bf16"
    with pytest.raises(NotImplementedError, match=r"^train\.clip_opt\.tower_arithmetic='bf16'"):
        train_config_from_opt(opt)


def test_clipscore_opt_takes_exact_and_split_and_refuses_the_rest(tmp_path):
    from satlas_super_resolution_amd import clipscore_metric as CM
    wfile = tmp_path / "w.pth"
    wfile.write_bytes(b"")
    kw = dict(clip_model="clip-ViT-B/16", clip_weights=str(wfile))
    assert "tower_arithmetic" in CM._OUR_KEYS
    absent = CM.check_clipscore_opt(**kw)
    assert CM.check_clipscore_opt(tower_arithmetic="exact", **kw) == absent == CM.check_clipscore_opt(tower_arithmetic="split", **kw)
    for bad in ("fp16", "Split", ""):
        with pytest.raises(NotImplementedError, match=f"calculate_clipscore.*tower_arithmetic={bad!r}"):
            CM.check_clipscore_opt(tower_arithmetic=bad, **kw)


def test_a_matrix_outside_the_fp16_domain_is_refused_by_name():
    from satlas_super_resolution_amd import clip_loss as CL
    from satlas_super_resolution_amd import clipscore_metric as CM
    from satlas_super_resolution_amd import linear_split as S
    state = LF.tower_state("B")
    state["blocks.1.fc1.weight"] = state["blocks.1.fc1.weight"].clone()
    state["blocks.1.fc1.weight"][3, 5] = -64.0
    with pytest.raises(ValueError, match=r"train\.clip_opt.*blocks\.1\.fc1\.weight has max\|w\| = 64"):
        CL.ClipLossModel(state, "cpu", tower_arithmetic="split")
    with pytest.raises(ValueError, match=r"calculate_clipscore.*blocks\.1\.fc1\.weight"):
        CM.CLIPVisualModel(state, "cpu", tower_arithmetic="split")
    clip = FX.tiny_state("clip")
    clip["proj"] = clip["proj"] * 1e4
    with pytest.raises(ValueError, match=r"calculate_clipscore.* proj has max"):
        CM.CLIPVisualModel(clip, "cpu", tower_arithmetic="split")
    S.check_split_domain([("m", torch.full((4, 4), 63.9))], "here")                     # inside the domain: accepted
    with pytest.raises(ValueError, match="here.*m has max"):
        S.check_split_domain([("m", torch.tensor([[float("nan")]]))], "here")
    with pytest.raises(NotImplementedError, match=r"^train\.clip_opt\.tower_arithmetic='half'"):
        CL.ClipLossModel(LF.tower_state("B"), "cpu", tower_arithmetic="half")
