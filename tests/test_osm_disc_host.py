"""CPU: OSMObjDiscriminator's object branch without a device - the plain-torch statement (satlas_super_resolution_amd/osm_reference.py)
against the fixtures the reference's own class produced (tools/make_osm_disc_golden.py), the closed-form attention backward against
autograd, the state_dict layout, the conditions on the fixtures, and the C ABI's argument checks.

Bounds: run in float64 the statement is held to the float64 records within 1e-9 * max|record| (both are float64 evaluations of the same
formulas in different association orders: ~1e-13 expected); run in float32, within the project's parity gate (conftest.parity_close).
key_conv.bias has a gradient that is zero in exact arithmetic (a constant added to every key shifts each softmax row uniformly): it is
never compared relatively but held to 1e-4 * max|gradient of key_conv.weight| in absolute terms."""
import ctypes as C

import pytest
import torch

import osm_disc_fixture as fx
from conftest import parity_close


@pytest.fixture(scope="module")
def fixture():
    head = fx.load_head()
    return dict(head=head, sd=fx.full_state(head), cases=[fx.load_case(i) for i in range(3)], grads=fx.load_grads())


def _branch_grads(sd, osm, w, dtype):
    from satlas_super_resolution_amd import osm_reference as R
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items() if k.startswith("o_")}
    o = osm.to(dtype).clone().requires_grad_(True)
    o_out = R.object_branch(p, o)
    (o_out * w.to(dtype)).sum().backward()
    g = {k: v.grad for k, v in p.items()}
    g["osm_objs"] = o.grad
    return o_out.detach(), g


def _key_bias_ok(g, ref_w, name):
    return float(g.abs().max()) <= 1e-4 * float(ref_w.abs().max()), f"{name}: {float(g.abs().max()):.3e} against max|dW| {float(ref_w.abs().max()):.3e}"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_object_branch_statement_matches_the_reference_records(fixture, dtype):
    sd, case, rec = fixture["sd"], fixture["cases"][0], fixture["grads"]["f64"]
    o_out, g = _branch_grads(sd, case["osm_objs"], case["w"], dtype)
    # the U-Net half does not feed o_out: the branch's gradients of sum(o_out * w) + mean(out) are those of the first term
    ref_out = case["train_o_out_f64"]
    names = [k for k, _ in fx.OBJ_KEYS] + ["osm_objs"]
    if dtype is torch.float64:
        assert float((o_out - ref_out).abs().max()) <= 1e-9 * float(ref_out.abs().max())
    else:
        assert parity_close(o_out, ref_out)
    for n in names:
        if n.endswith("key_conv.bias"):
            ok, msg = _key_bias_ok(g[n], rec[n.replace(".bias", ".weight")], n)
            assert ok, msg
            continue
        if dtype is torch.float64:
            err = float((g[n] - rec[n]).abs().max()) / float(rec[n].abs().max())
            assert err <= 1e-9, (n, err)
        else:
            assert parity_close(g[n], rec[n]), n
    for ci in (1, 2):                                   # the outputs-only cases: other token grids, a 1 x 1 o_out
        c = fixture["cases"][ci]
        from satlas_super_resolution_amd import osm_reference as R
        with torch.no_grad():
            o = R.object_branch({k: v.to(dtype) for k, v in sd.items()}, c["osm_objs"].to(dtype))
        ref = c["eval_o_out_f64"]
        assert o.shape == ref.shape
        if dtype is torch.float64:
            assert float((o - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
        else:
            assert parity_close(o, ref)


@pytest.mark.parametrize("B,H,W,Cc", [(2, 2, 2, 32), (3, 4, 8, 128), (1, 8, 8, 64)])
def test_closed_form_attention_backward_equals_autograd_in_float64(B, H, W, Cc):
    from satlas_super_resolution_amd import osm_reference as R
    x, dy, p = fx.attention_case(H * 100 + W, B, H * W, Cc)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xl = x.clone().requires_grad_(True)
    y, saved = R.attention_forward(xl, leaves)
    peak = float(saved["a"].detach().max(dim=2).values.mean())
    assert 0.1 <= peak <= 0.9, peak                      # neither uniform nor one-hot
    (y * dy).sum().backward()
    with torch.no_grad():
        y2, s2 = R.attention_forward(x, p)
        got = R.attention_backward(dy, x, p, s2)
    auto = dict(dx=xl.grad, dwq=leaves["wq"].grad, dbq=leaves["bq"].grad, dwk=leaves["wk"].grad, dbk=leaves["bk"].grad,
                dwv=leaves["wv"].grad, dbv=leaves["bv"].grad, dgamma=leaves["gamma"].grad)
    for n in R.ATTN_GRADS:
        if n == "dbk":
            assert float(got[n].abs().max()) <= 1e-9 * float(auto["dwk"].abs().max()) and float(auto[n].abs().max()) <= 1e-9 * float(auto["dwk"].abs().max())
            continue
        err = float((got[n] - auto[n]).abs().max()) / float(auto[n].abs().max())
        assert err <= 1e-12, (n, err)
    # the NCHW wrapper walks tokens as h * W + w
    xn = x.transpose(1, 2).reshape(B, Cc, H, W)
    assert torch.equal(R.self_attention(xn, p), y2.transpose(1, 2).reshape(B, Cc, H, W))


def test_state_dict_keys_shapes_and_order_are_the_references(fixture):
    from satlas_super_resolution_amd.archs.osm_obj_discriminator_arch import OSMObjDiscriminator
    from satlas_super_resolution_amd.registry import ARCH_REGISTRY
    head = fixture["head"]
    assert ARCH_REGISTRY.get("OSMObjDiscriminator") is OSMObjDiscriminator
    net = OSMObjDiscriminator(**head["kwargs"])
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(got) == 50 and got == head["keys"]
    assert got == fx.OBJ_KEYS + fx.unet_keys(head["kwargs"]["num_feat"], head["kwargs"]["num_in_ch"])
    assert [k for k, _ in net.named_parameters()] == [k for k, _ in got if not k.endswith(("weight_u", "weight_v"))]
    net.load_state_dict(fixture["sd"], strict=True)      # the checkpoint the reference's class saved
    for k, v in net.state_dict().items():
        assert torch.equal(v, fixture["sd"][k]), k
    assert sum(p.numel() for k, p in net.named_parameters() if k.startswith("o_")) == 765_859 == head["n_object_parameters"]
    with pytest.raises(NotImplementedError, match="bf16"):
        OSMObjDiscriminator(27, compute_dtype="bf16")
    # the network_d block of the shipped option file builds
    import json
    import os
    from conftest import GOLDEN
    opt = json.load(open(os.path.join(GOLDEN, "ssr_options.json")))["osm_obj_esrgan.yml"]["network_d"]
    kw = {k: v for k, v in opt.items() if k != "type"}
    big = ARCH_REGISTRY.get(opt["type"])(**kw)
    assert big.num_feat == 64 and big.num_in_ch == 27 and len(big.state_dict()) == 50


def test_the_fixtures_meet_their_conditions(fixture):
    head, sd, cases, grads = fixture["head"], fixture["sd"], fixture["cases"], fixture["grads"]
    # the rule reproduces: exact float32 values, gammas and the last bias as stated
    assert float(sd["o_attention1.gamma"]) == pytest.approx(0.7) and float(sd["o_attention2.gamma"]) == pytest.approx(-0.4)
    assert float(sd["o_conv4.bias"]) == pytest.approx(0.05)
    w = sd["o_conv3.weight"]
    assert w.dtype == torch.float32 and float(w.abs().max()) <= 3.0 / (128 * 16) ** 0.5 and float(w.abs().max()) > 2.9 / (128 * 16) ** 0.5
    sd64 = {k: v.double() for k, v in sd.items()}
    pooled = fx.branch_stats(sd64, [c["osm_objs"].double() for c in cases])
    first = fx.branch_stats(sd64, [cases[0]["osm_objs"].double()])
    assert fx.stats_ok(pooled), pooled
    assert fx.stats_ok(first), first
    assert all(bool((c["eval_o_out"] > 0).any()) for c in cases)          # no case compares zeros with zeros
    assert pooled == pytest.approx(cases[0]["stats_pooled"]) and first == pytest.approx(cases[0]["stats_case0"])
    assert (cases[0]["w"] > 0).any() and (cases[0]["w"] < 0).any()
    # no test rests on a ReLU decision float32 cannot make: the reference's own float32 gradients are within the gate of its float64 ones
    for n, g64 in grads["f64"].items():
        g32 = grads["f32"][n]
        assert g32.dtype == torch.float32 and g64.dtype == torch.float64
        if n.endswith("key_conv.bias"):
            kw = grads["f64"][n.replace(".bias", ".weight")]
            assert float(g64.abs().max()) <= 1e-9 * float(kw.abs().max())          # recorded as zero
            assert float(g32.abs().max()) <= 1e-4 * float(kw.abs().max())
            continue
        d = float((g32.double() - g64).abs().max()) / float(g64.abs().max())
        assert d <= fx.GRAD_GATE, (n, d)
        assert float(g64.abs().max()) > 0, n
    assert cases[0]["key_conv_bias_grad_is_zero"] is True
    assert cases[1]["eval_o_out"].shape == (3, 1, 1, 2) and cases[2]["eval_o_out"].shape == (1, 1, 1, 1)


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    return hip, hip.lib()


def test_attention_entries_are_exported_and_reject_bad_descriptors_without_a_launch():
    hip, L = _lib()
    for s in ("ssr_self_attention_fwd", "ssr_self_attention_bwd", "ssr_self_attention_save_floats", "ssr_self_attention_scratch_floats",
              "ssr_relu_bwd"):
        assert s in hip.ABI_SYMBOLS and hasattr(L, s)
    from satlas_super_resolution_amd import build
    assert "attention.hip" in build.SOURCES
    assert L.ssr_abi_version() == 3
    assert L.ssr_self_attention_save_floats(64, 128) == 64 * 64 + 2 * 64 * 16 + 2 * 64 * 128
    assert L.ssr_self_attention_scratch_floats(16, 64, 128) >= 16 * 64 * 160 + 16
    fake = 1 << 20                      # a 16-byte aligned address that is never dereferenced: every call below fails its checks first

    def desc(**over):
        d = hip.AttnDesc()
        d.Bo, d.N, d.C = 2, 16, 128
        v = hip.View(fake, 128, 0)
        d.x, d.y, d.dy, d.dx = v, v, v, v
        for f in ("wq", "bq", "wk", "bk", "wv", "bv", "gamma", "save", "scratch", "dwq", "dbq", "dwk", "dbk", "dwv", "dbv", "dgamma"):
            setattr(d, f, fake)
        for k, val in over.items():
            setattr(d, k, val)
        return d

    bad = [dict(Bo=0), dict(C=124), dict(C=0), dict(N=12), dict(N=128), dict(N=0), dict(x=hip.View(None, 128, 0)),
           dict(x=hip.View(fake + 4, 128, 0)), dict(x=hip.View(fake, 130, 0)), dict(x=hip.View(fake, 128, 2)), dict(x=hip.View(fake, 64, 0)),
           dict(wq=None), dict(wv=fake + 8), dict(gamma=None)]
    for fn in (L.ssr_self_attention_fwd, L.ssr_self_attention_bwd):
        assert fn(None, None) == -1
        for over in bad:
            assert fn(C.byref(desc(**over)), None) == -1, over
    assert L.ssr_self_attention_fwd(C.byref(desc(y=hip.View(None, 128, 0))), None) == -1
    assert L.ssr_self_attention_fwd(C.byref(desc(bq=None)), None) == -1
    assert L.ssr_self_attention_fwd(C.byref(desc(save=fake + 4)), None) == -1
    for over in (dict(dy=hip.View(None, 128, 0)), dict(dx=hip.View(fake, 128, 132)), dict(save=None), dict(scratch=None),
                 dict(dwq=None), dict(dgamma=None), dict(dwv=fake + 4)):
        assert L.ssr_self_attention_bwd(C.byref(desc(**over)), None) == -1, over
    # valid but not instantiated: -2, still without a launch
    assert L.ssr_self_attention_fwd(C.byref(desc(C=72, x=hip.View(fake, 128, 0))), None) == -2
    assert L.ssr_self_attention_fwd(C.byref(desc(C=512, x=hip.View(fake, 512, 0), y=hip.View(fake, 512, 0))), None) == -2
    v = hip.View(fake, 8, 0)
    assert L.ssr_relu_bwd(hip.View(None, 8, 0), v, v, 4, 1, None) == -1
    assert L.ssr_relu_bwd(v, v, v, 0, 1, None) == -1
    assert L.ssr_relu_bwd(v, v, v, 4, 9, None) == -1


def test_unsupported_crop_sizes_are_refused_by_name():
    from satlas_super_resolution_amd.archs.osm_obj_discriminator_arch import OSMObjDiscriminator
    net = OSMObjDiscriminator(27, num_feat=8)
    for shape in ((2, 3, 24, 32), (2, 3, 64, 64), (2, 4, 32, 32)):
        with pytest.raises(ValueError, match=str(shape[2])):
            net(torch.zeros(1, 27, 16, 16), torch.zeros(*shape))
