"""CPU: the LPIPS metric's definition (lpips_metric.lpips_reference), its weight layouts and the option handling of
`calculate_lpips`.  No device work: the GPU path is tests/test_gpu_lpips.py."""
import pytest
import torch

from satlas_super_resolution_amd import lpips_metric as LM


@pytest.fixture(scope="module")
def state():
    return LM.lpips_random_state(3)


@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(11)
    a = torch.randint(0, 256, (2, 16, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (2, 16, 32, 3), generator=g, dtype=torch.uint8)
    return a, b


def test_layer_table_is_vgg16():
    layers = LM.vgg16_layers()
    assert [l[1] for l in layers] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [l[3] for l in layers] == [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
    assert [l[0] for l in layers if l[4]] == ["conv2_1", "conv3_1", "conv4_1", "conv5_1"]
    names = [l[0] for l in layers]
    # every tap but the last sits in front of a pooling
    assert all(layers[names.index(t) + 1][4] for t in LM.LPIPS_TAPS[:-1]) and names[-1] == LM.LPIPS_TAPS[-1]
    assert [s.name for s in LM.vgg16_specs()] == [f"features.{i}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)]


def test_hand_computed_one_layer():
    """pixel 0: (3, 4) / 5 = (.6, .8) against (0, 5) / 5 = (0, 1): 2 * .36 + 3 * .04 = .84;  pixel 1: the zero-norm pixel (0, 0) -> 0 / 1e-10
    = 0 against (1, 0): 2 * 1 = 2;  mean = 1.42"""
    f0 = torch.tensor([[[[3.0, 0.0]], [[4.0, 0.0]]]], dtype=torch.float64)          # [1, 2, 1, 2]
    f1 = torch.tensor([[[[0.0, 1.0]], [[5.0, 0.0]]]], dtype=torch.float64)
    w = torch.tensor([2.0, 3.0])
    d = LM.lpips_from_features({"t": f0}, {"t": f1}, {"t": w})
    assert d.shape == (1,) and float(d[0]) == pytest.approx(1.42, rel=1e-9)
    # two taps add
    d2 = LM.lpips_from_features({"t": f0, "u": f0[:, :, :, :1]}, {"t": f1, "u": f1[:, :, :, :1]}, {"t": w, "u": w})
    assert float(d2[0]) == pytest.approx(1.42 + 0.84, rel=1e-9)


def test_zero_norm_pixel_contributes_nothing():
    z = torch.zeros(1, 4, 2, 2, dtype=torch.float64)
    assert float(LM.lpips_from_features({"t": z}, {"t": z}, {"t": torch.ones(4)})[0]) == 0.0
    f = z.clone()
    f[0, :, 0, 0] = torch.tensor([1.0, 2.0, 2.0, 0.0])               # one live pixel, identical in both: still 0
    assert float(LM.lpips_from_features({"t": f}, {"t": f}, {"t": torch.ones(4)})[0]) == 0.0
    g = f.clone()
    g[0, :, 0, 0] = torch.tensor([0.0, 0.0, 0.0, 3.0])               # unit vectors (1,2,2,0)/3 and (0,0,0,1): squared distance 2, over 4 pixels
    assert float(LM.lpips_from_features({"t": f}, {"t": g}, {"t": torch.ones(4)})[0]) == pytest.approx(0.5, rel=1e-9)


def test_reference_identity_and_symmetry(state, images):
    a, b = images
    assert torch.equal(LM.lpips_reference(a, a, state), torch.zeros(2, dtype=torch.float64))
    dab, dba = LM.lpips_reference(a, b, state), LM.lpips_reference(b, a, state)
    assert dab.shape == (2,) and dab.dtype == torch.float64 and bool((dab > 0).all())
    assert torch.allclose(dab, dba, rtol=1e-12, atol=0)
    # per image: the batch is N independent pairs
    assert torch.allclose(LM.lpips_reference(a[1:], b[1:], state), dab[1:], rtol=1e-12, atol=0)


def test_bgr_and_normalize_give_four_numbers(state, images):
    a, b = images
    vals = [float(LM.lpips_reference(a[:1], b[:1], state, bgr=bgr, normalize=nz)[0]) for bgr in (True, False) for nz in (False, True)]
    assert len({round(v, 12) for v in vals}) == 4, vals


def test_scaled_input_order_of_operations():
    u = torch.tensor([[[[10, 128, 255]]]], dtype=torch.uint8)
    x = LM.lpips_scaled_input(u, bgr=True, normalize=True, dtype=torch.float64)[0, :, 0, 0]
    want = [((2 * v / 255 - 1) - float(torch.tensor(s, dtype=torch.float32))) / float(torch.tensor(c, dtype=torch.float32))
            for v, s, c in zip((255, 128, 10), LM.LPIPS_SHIFT, LM.LPIPS_SCALE)]
    assert x.tolist() == pytest.approx(want, rel=1e-14)
    y = LM.lpips_scaled_input(u, bgr=False, normalize=False, dtype=torch.float64)[0, :, 0, 0]
    assert float(y[0]) == pytest.approx((10 / 255 + 0.030) / 0.458, rel=1e-7)


def _as_package_state(state):
    """what lpips.LPIPS(net='vgg').state_dict() holds [recalled]: net.slice{s}.{idx}.*, lin{k}.model.1.weight, lins.{k}.*, scaling_layer.*"""
    slices = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
    sd = {"scaling_layer.shift": torch.tensor(LM.LPIPS_SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(LM.LPIPS_SCALE).view(1, 3, 1, 1)}
    for s, idxs in slices.items():
        for i in idxs:
            sd[f"net.slice{s}.{i}.weight"] = state[f"features.{i}.weight"]
            sd[f"net.slice{s}.{i}.bias"] = state[f"features.{i}.bias"]
    for k in range(5):
        sd[f"lin{k}.model.1.weight"] = state[f"lin{k}"].view(1, -1, 1, 1)
        sd[f"lins.{k}.model.1.weight"] = state[f"lin{k}"].view(1, -1, 1, 1)
    return sd


def test_three_weight_layouts_load_identically(state, tmp_path):
    torch.save(state, tmp_path / "flat.pth")
    torch.save(_as_package_state(state), tmp_path / "combined.pth")
    tv = {k: v for k, v in state.items() if k.startswith("features.")}
    tv["classifier.0.weight"] = torch.zeros(4, 4)                           # torchvision's file has the classifier too
    torch.save(tv, tmp_path / "vgg16.pth")
    torch.save({f"lin{k}.model.1.weight": state[f"lin{k}"].view(1, -1, 1, 1) for k in range(5)}, tmp_path / "lin.pth")
    flat = LM.load_lpips_state(str(tmp_path / "flat.pth"))
    comb = LM.load_lpips_state(str(tmp_path / "combined.pth"))
    two = LM.load_lpips_state(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth"))
    assert sorted(flat) == sorted(state) and len(flat) == 26 + 5
    for k, v in state.items():
        assert torch.equal(flat[k], v) and torch.equal(comb[k], v) and torch.equal(two[k], v), k
        assert flat[k].shape == v.shape


def test_missing_and_misshaped_keys_raise_by_name(state, tmp_path):
    sd = _as_package_state(state)
    del sd["net.slice3.12.bias"]
    torch.save(sd, tmp_path / "a.pth")
    with pytest.raises(KeyError, match=r"features\.12\.bias"):
        LM.load_lpips_state(str(tmp_path / "a.pth"))
    sd = _as_package_state(state)
    del sd["lin2.model.1.weight"]
    torch.save(sd, tmp_path / "b.pth")
    with pytest.raises(KeyError, match="lin2"):
        LM.load_lpips_state(str(tmp_path / "b.pth"))
    tv = {k: v for k, v in state.items() if k.startswith("features.")}
    torch.save(tv, tmp_path / "c.pth")
    with pytest.raises(KeyError, match="lin0"):                                  # the backbone alone has no linear layers
        LM.load_lpips_state(str(tmp_path / "c.pth"))
    bad = dict(state)
    bad["features.5.weight"] = torch.zeros(128, 64, 1, 1)
    torch.save(bad, tmp_path / "d.pth")
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        LM.load_lpips_state(str(tmp_path / "d.pth"))
    bad = dict(state)
    bad["lin4"] = torch.zeros(256)
    torch.save(bad, tmp_path / "e.pth")
    with pytest.raises(ValueError, match="lin4"):
        LM.load_lpips_state(str(tmp_path / "e.pth"))


def test_random_state_is_seeded_and_lins_are_non_negative():
    a, b, c = LM.lpips_random_state(5), LM.lpips_random_state(5), LM.lpips_random_state(6)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a["features.0.weight"], c["features.0.weight"])
    assert all(float(a[f"lin{k}"].min()) >= 0.0 and float(a[f"lin{k}"].max()) < 1.0 for k in range(5))
    assert [a[f"lin{k}"].numel() for k in range(5)] == [64, 128, 256, 512, 512]


def test_option_handling(state, tmp_path, monkeypatch):
    from satlas_super_resolution_amd import metrics as M
    assert M.METRICS["calculate_lpips"] is LM.calculate_lpips and M.METRIC_CHECKS["calculate_lpips"] is LM.check_lpips_opt
    monkeypatch.delenv("SSR_LPIPS_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)                                         # no experiments/pretrained_models/lpips_vgg.pth here
    with pytest.raises(NotImplementedError, match="lpips_model") as e:
        LM.check_lpips_opt(lpips_model="alexnet")
    assert "alexnet" in str(e.value)
    with pytest.raises(NotImplementedError, match="window_size"):
        LM.check_lpips_opt(lpips_model="vgg", window_size=7)
    with pytest.raises(NotImplementedError, match=r"^metric type 'calculate_lpips': ") as e:
        LM.check_lpips_opt(lpips_model="vgg", crop_border=4, test_y_channel=False, input_order="HWC", better="lower")
    msg = str(e.value)
    assert "lpips_weights" in msg and "SSR_LPIPS_WEIGHTS" in msg and LM.LPIPS_PRETRAIN_PATH in msg and "no silent random network" in msg
    # the metric entry raises the same before it touches its images
    with pytest.raises(NotImplementedError, match="calculate_lpips"):
        LM.calculate_lpips(None, None, lpips_model="vgg")
    with pytest.raises(FileNotFoundError, match="lpips_weights"):
        LM.check_lpips_opt(lpips_model="vgg", lpips_weights=str(tmp_path / "nope.pth"))
    with pytest.raises(ValueError, match="lin_path"):
        LM.check_lpips_opt(lpips_model="vgg", vgg16_path=str(tmp_path / "nope.pth"))
    # lookup order: the keys, then the environment, then the default place
    for name in ("key.pth", "env.pth", "vgg16.pth", "lin.pth"):
        torch.save({}, tmp_path / name)
    (tmp_path / "experiments" / "pretrained_models").mkdir(parents=True)
    torch.save({}, tmp_path / LM.LPIPS_PRETRAIN_PATH)
    real = lambda p: str((tmp_path / p).resolve())                       # noqa: E731
    assert LM.check_lpips_opt(lpips_model="vgg") == (real(LM.LPIPS_PRETRAIN_PATH), None)
    monkeypatch.setenv("SSR_LPIPS_WEIGHTS", str(tmp_path / "env.pth"))
    assert LM.check_lpips_opt(lpips_model="vgg", rgb=True, normalize=True) == (real("env.pth"), None)
    assert LM.check_lpips_opt(lpips_model="vgg", lpips_weights=str(tmp_path / "key.pth")) == (real("key.pth"), None)
    assert LM.check_lpips_opt(lpips_model="vgg", vgg16_path=str(tmp_path / "vgg16.pth"), lin_path=str(tmp_path / "lin.pth")) == \
        (real("vgg16.pth"), real("lin.pth"))


def test_plan_rejects_sizes_that_do_not_pool_four_times():
    with pytest.raises(ValueError, match="24"):
        LM.LPIPSPlan(1, 24, 32, None)


def test_reference_against_the_lpips_package(tmp_path):
    """The only check that can remove the [recalled] marks ("LPIPS metric"): lpips_reference against the lpips package
    with the package's own weights.  Skips where the package, or the torchvision VGG16 file it needs, is not installed; it never
    downloads."""
    lpips = pytest.importorskip("lpips")
    import glob
    import os
    hub = os.path.join(torch.hub.get_dir(), "checkpoints")
    if not glob.glob(os.path.join(hub, "vgg16-*.pth")):
        pytest.skip("torchvision's vgg16 checkpoint is not in the local hub cache (no download here)")
    net = lpips.LPIPS(net="vgg", pretrained=True, verbose=False).eval()
    torch.save(net.state_dict(), tmp_path / "pkg.pth")
    st = LM.load_lpips_state(str(tmp_path / "pkg.pth"))
    g =torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (1, 32, 32, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (1, 32, 32, 3), generator=g, dtype=torch.uint8)
    to = lambda u: u.permute(0, 3, 1, 2).float() / 255                   # noqa: E731
    with torch.no_grad():
        quirk = float(net(to(a.flip(-1)), to(b.flip(-1))))              # the reference's feed: BGR, [0, 1]
        doc = float(net(to(a), to(b), normalize=True))                   # the package's documented use
    assert float(LM.lpips_reference(a, b, st)[0]) == pytest.approx(quirk, rel=1e-4)
    assert float(LM.lpips_reference(a, b, st, bgr=False, normalize=True)[0]) == pytest.approx(doc, rel=1e-4)
