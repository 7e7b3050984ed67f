"""CPU: L2Model's networks without a GPU - the CPU statement (l2_reference.py) against the fixtures recorded from the reference's own
SRCNN and HighResNet (tools/make_l2_golden.py), the checkpoint layout of archs/l2_archs.py, option handling and refusals, and the
host restatement of the dropout generator."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

FILES = {"SRCNN": "l2_srcnn_tiny", "HighResNet": "l2_highresnet_tiny"}
_CACHE = {}


def fixture(arch, case=None):
    name = FILES[arch] + ("" if case is None else f"_case{case}")
    if name not in _CACHE:
        _CACHE[name] = torch.load(os.path.join(GOLDEN, name + ".pt"), map_location="cpu", weights_only=False)
    return _CACHE[name]


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", [0, 1])
@pytest.mark.parametrize("arch", ["SRCNN", "HighResNet"])
def test_cpu_statement_reproduces_the_reference_fixture(arch, case):
    """float64 evaluation against the fixture's float32 values, 1e-5 * max|ref|: eval output, training output with the recorded masks,
    the loss terms and every parameter gradient"""
    from satlas_super_resolution_amd import l2_reference as R
    fn = R.srcnn_reference if arch == "SRCNN" else R.highresnet_reference
    head, c = fixture(arch), fixture(arch, case)
    names = head["param_names"]
    leaves = {k: head["state_dict"][k].double().requires_grad_(True) for k in names}
    # every state_dict key resolves to the leaf of the parameter it names: SRCNN's fusion.* aliases, HighResNet's shared block
    from satlas_super_resolution_amd.archs import l2_archs
    net = getattr(l2_archs, arch)(**head["kwargs"])
    canon = {id(p): k for k, p in net.named_parameters()}
    sd = {k: leaves[canon[id(p)]] for k, p in net.named_parameters(remove_duplicate=False)}
    assert set(sd) == set(head["state_dict"])
    x = c["x"].double()
    with torch.no_grad():
        assert _rel(fn(sd, x), c["eval_out"]) < 1e-5
    out = fn(sd, x, c["masks"])
    assert tuple(out.shape) == tuple(c["train_out"].shape) and _rel(out.detach(), c["train_out"]) < 1e-5
    loss = R.l2_loss_reference(out.squeeze(1), c["gt"].double())
    for k, v in c["loss"].items():
        assert abs(float(loss[k]) - v) <= 1e-5 * abs(v), k
    loss["tot_loss"].backward()
    for k, ref in c["grads"].items():
        if ref is None:
            assert leaves[k].grad is None, k
        else:
            assert _rel(leaves[k].grad, ref) < 1e-5, k
    assert len(c["masks"]) == len(R.dropout_site_shapes(arch, 2, x.shape[1], x.shape[3], x.shape[4], 32, 1))
    assert [tuple(m.shape) for m in c["masks"]] == R.dropout_site_shapes(arch, 2, x.shape[1], x.shape[3], x.shape[4], 32, 1)


@pytest.mark.parametrize("arch", ["SRCNN", "HighResNet"])
def test_state_dict_layout_is_the_references(arch):
    from satlas_super_resolution_amd.archs import l2_archs
    head = fixture(arch)
    net = getattr(l2_archs, arch)(**head["kwargs"])
    sd, ref = net.state_dict(), head["state_dict"]
    assert list(sd) == list(ref)
    assert all(tuple(sd[k].shape) == tuple(ref[k].shape) for k in ref)
    assert [k for k, _ in net.named_parameters()] == head["param_names"]
    assert sum(p.numel() for p in net.parameters()) == head["n_parameters"]
    net.load_state_dict(ref, strict=True)
    m = "mask_encoder.1.doubleconv2d."
    assert tuple(sd[m + "0.weight"].shape) == (1, 0, 3, 3) and tuple(sd[m + "4.weight"].shape) == (1, 1, 3, 3)
    assert [tuple(sd[m + k].shape) for k in ("0.bias", "2.weight", "4.bias", "6.weight")] == [(1,)] * 4
    d = "doubleconv2d.doubleconv2d.0.weight"
    if arch == "SRCNN":        # the fusion aliases are the same storage
        assert sd["fusion.0.doubleconv2d.0.weight"].data_ptr() == sd[d].data_ptr()
        assert sd["fusion.1.0.residualblock.doubleconv2d.4.bias"].data_ptr() == sd["residualblocks.0.residualblock.doubleconv2d.4.bias"].data_ptr()
        assert all(not k.startswith(("doubleconv2d.", "residualblocks.")) or k in net.live_keys() for k in head["param_names"])
    else:                       # one shared FusionBlock listed once per level; SRCNN's fusion parameters are dead
        a, b = "fusion.fusion.0.fuse.1.weight", "fusion.fusion.1.fuse.1.weight"
        assert sd[a].data_ptr() == sd[b].data_ptr()
        live = set(net.live_keys())
        dead = [k for k in head["param_names"] if k not in live]
        assert dead and all(k.startswith(("mask_encoder.", "doubleconv2d.", "residualblocks.")) for k in dead)
        c = fixture(arch, 0)
        assert {k for k, g in c["grads"].items() if g is None} == set(dead)      # exactly the parameters the reference gives no gradient


def test_parameter_count_at_the_shipped_highresnet_size():
    from satlas_super_resolution_amd.archs.l2_archs import HighResNet
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["highresnet_s2naip_urban.yml"]["network_g"]
    net = HighResNet(**{k: v for k, v in opt.items() if k != "type"})
    assert sum(p.numel() for p in net.parameters()) == 3_249_019             # what the reference's model prints


@pytest.mark.parametrize("name,arch", [("srcnn_s2naip_urban.yml", "SRCNN"), ("highresnet_s2naip_urban.yml", "HighResNet")])
def test_shipped_option_files_build_through_l2model_option_handling(name, arch):
    from satlas_super_resolution_amd import models  # noqa: F401
    from satlas_super_resolution_amd.models.ssr_l2_model import validate_options
    from satlas_super_resolution_amd.registry import MODEL_REGISTRY
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))[name]
    assert opt["model_type"] == "L2Model" and MODEL_REGISTRY.get("L2Model").__name__ == "L2Model"
    net, spec, sched, ema = validate_options(opt)
    assert type(net).__name__ == arch and spec["type"] == "Adam" and spec["betas"] == (0.9, 0.99) and ema == 0.0
    assert sched.lr(spec["lr"], 1) == spec["lr"] and sched.lr(spec["lr"], 400002) == 0.5 * spec["lr"]
    assert net.kwargs["hidden_channels"] == 128 and net.kwargs["revisits"] == 8


BASE = dict(in_channels=3, mask_channels=0, revisits=4, hidden_channels=32, out_channels=3, kernel_size=3, residual_layers=1,
            output_size=32, zoom_factor=4, sr_kernel_size=1)


@pytest.mark.parametrize("arch", ["SRCNN", "HighResNet"])
@pytest.mark.parametrize("key,value", [("mask_channels", 1), ("use_reference_frame", True), ("kernel_size", 5), ("sr_kernel_size", 3),
                                       ("compute_dtype", "bf16"), ("compute_dtype", "fp32x3"), ("compute_dtype", "fp32h"),
                                       ("compute_dtype", "fp32f"), ("hidden_channels", 24)])
def test_unsupported_constructor_arguments_raise_by_name(arch, key, value):
    from satlas_super_resolution_amd.archs import l2_archs
    with pytest.raises(NotImplementedError, match=key):
        getattr(l2_archs, arch)(**dict(BASE, **{key: value}))
    # and through the model's option handling
    from satlas_super_resolution_amd.models.ssr_l2_model import validate_options
    with pytest.raises(NotImplementedError, match=key):
        validate_options({"model_type": "L2Model", "network_g": dict(BASE, type=arch, **{key: value}), "train": {"optim_g": {"type": "Adam", "lr": 1e-4}}})


def test_output_size_that_needs_resampling_raises_by_name():
    from satlas_super_resolution_amd.archs.l2_archs import check_output_size
    check_output_size(32, 4, 8, 8)
    check_output_size([24, 40], 4, 6, 10)
    check_output_size((24, 40), 4, 6, 10)
    for osz, h, w in ((64, 8, 8), (24, 6, 10), ([40, 24], 6, 10), ([32, 32], 8, 9)):
        with pytest.raises(NotImplementedError, match="output_size"):
            check_output_size(osz, 4, h, w)
    from satlas_super_resolution_amd.archs.l2_archs import SRCNN
    with pytest.raises(NotImplementedError, match="output_size"):
        SRCNN(**dict(BASE, output_size="big"))


def test_other_refusals_name_what_they_refuse(monkeypatch):
    from satlas_super_resolution_amd.models.ssr_l2_model import validate_options
    opt = {"model_type": "L2Model", "network_g": dict(BASE, type="SRCNN"), "train": {"optim_g": {"type": "Adam", "lr": 1e-4}}}
    validate_options(opt)
    with pytest.raises(NotImplementedError, match="SSR_RRDBNet"):
        validate_options(dict(opt, network_g={"type": "SSR_RRDBNet", "num_in_ch": 24, "num_out_ch": 3}))
    with pytest.raises(NotImplementedError, match="compute_dtype"):
        validate_options(dict(opt, compute_dtype="fp32h"))
    with pytest.raises(NotImplementedError, match="Adamax"):
        validate_options(dict(opt, train={"optim_g": {"type": "Adamax", "lr": 1e-4}}))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="L2Model"):
        validate_options(opt)
    monkeypatch.delenv("WORLD_SIZE")
    # no GPU path for a CPU tensor, and none silently taken
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.archs.l2_archs import SRCNN
    with pytest.raises(hip.HipLibraryError):
        SRCNN(**BASE)(torch.rand(1, 4, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="mask"):
        SRCNN(**BASE)(torch.rand(1, 4, 3, 8, 8), mask=torch.zeros(1, 4, 1, 8, 8))


def test_dropout_generator_host_restatement():
    from satlas_super_resolution_amd import l2_reference as R
    n = 1 << 20
    lo, hi = 0.5 - 4 * 0.5 / 1024, 0.5 + 4 * 0.5 / 1024              # 4 sigma of a fair coin over 2^20 draws
    base = dict(seed=0x0123456789ABCDEF, step=7, layer=2)
    words = R.philox_keep_bits(n_words=n // 32, **base)
    assert words.dtype == np.uint32 and words.shape == (n // 32,)
    assert np.array_equal(words, R.philox_keep_bits(n_words=n // 32, **base))                  # the same key, the same bits
    assert np.array_equal(words[:64], R.philox_keep_bits(n_words=64, **base))                  # a prefix does not depend on the length
    a = R.unpack_bits(words, n)
    assert lo <= a.mean() <= hi
    for field, other in (("seed", base["seed"] ^ 1), ("seed", base["seed"] ^ (1 << 40)), ("step", 8), ("layer", 3)):
        b = R.unpack_bits(R.philox_keep_bits(n_words=n // 32, **dict(base, **{field: other})), n)
        assert lo <= b.mean() <= hi and lo <= (a == b).mean() <= hi, field                      # independent streams agree on half
    # Random123's known answer for Philox4x32-10 with a zero counter and a zero key
    assert [int(v) for v in R.philox_keep_bits(0, 0, 0, 4)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # packing: NCHW bool mask -> NHWC element order, bit e & 31 of word e >> 5
    m = torch.rand(2, 8, 3, 5) < 0.5
    w = R.pack_mask_nhwc(m)
    assert w.size == R.mask_words(m.numel()) and w.size % 4 == 0
    assert np.array_equal(R.unpack_bits(w, m.numel()), m.permute(0, 2, 3, 1).reshape(-1).numpy())


def test_kernel_restatements_are_the_transpose_pair():
    """prelu_reflect_bwd_np is the gradient of prelu_reflect_fwd_np (float64 autograd of the same composition), corners included"""
    import torch.nn.functional as F
    from satlas_super_resolution_amd import l2_reference as R
    rng = np.random.default_rng(0)
    for H, W in ((2, 2), (3, 3), (3, 5), (4, 4), (6, 10)):
        pre = rng.standard_normal((2, H, W, 8)).astype(np.float32)
        keep = rng.random((2, H, W, 8)) < 0.5
        g = rng.standard_normal((2, H + 2, W + 2, 8)).astype(np.float32)
        x = torch.tensor(pre, dtype=torch.float64, requires_grad=True)
        a = torch.tensor(0.2, dtype=torch.float64, requires_grad=True)
        v = torch.where(x > 0, x, a * x) * torch.tensor(keep) * 2
        vp = F.pad(v.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
        assert np.allclose(vp.detach().numpy(), R.prelu_reflect_fwd_np(pre, np.float32(0.2), keep, None, 1), atol=1e-6)
        (vp * torch.tensor(g, dtype=torch.float64)).sum().backward()
        dpre, terms = R.prelu_reflect_bwd_np(pre, np.float32(0.2), g, 1, keep)
        assert np.allclose(dpre, x.grad.numpy(), atol=1e-5) and abs(terms.sum() - float(a.grad)) < 1e-4
