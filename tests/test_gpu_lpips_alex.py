"""GPU: the AlexNet backbone of the LPIPS metric (`lpips_model: alexnet`): the two C-ABI entries of csrc/conv_direct.hip on their
own (ssr_conv_direct against float64 F.conv2d within a derived bound, ssr_maxpool3s2_fwd bit-exact), the whole metric through
lpips_distance against lpips_reference(..., net="alex") in float64, and `calculate_lpips` through the model plugin's test pipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of fp32


# ------------------------------------------------------------------ ssr_conv_direct
# (name, K, stride, pad, cin valid, cin contracted, cout, N, Hi, Wi)
CONV_CASES = [
    ("conv1 35x47", 11, 4, 2, 3, 8, 64, 2, 35, 47),           # stride remainders 0 and 3, uneven sides
    ("conv1 31x31", 11, 4, 2, 3, 8, 64, 1, 31, 31),
    ("conv2 8x11", 5, 1, 2, 64, 64, 192, 2, 8, 11),
    ("conv2 3x3", 5, 1, 2, 64, 64, 192, 2, 3, 3),             # grid smaller than the kernel: every tap of every output touches the border
    ("conv3 1x2", 3, 1, 1, 192, 192, 384, 2, 1, 2),
    ("7x7 s2 9x10", 7, 2, 3, 16, 16, 32, 2, 9, 10),           # outside the network: nothing is hard-coded
    ("3x3 2x40", 3, 1, 1, 8, 8, 32, 2, 2, 40),                # 40 output columns: two pixel tiles, the second partly filled
]


def _conv_direct(x, wd, bias, N, Hi, Wi, cin, cout, K, stride, pad, relu, xcs, xcoff, ycs, ycoff):
    """x: float32 [N, Hi, Wi, cin] on the host -> the whole output buffer [N, Ho, Wo, ycs] (NaN outside the slice) as numpy"""
    from satlas_super_resolution_amd import hip
    Ho, Wo = (Hi + 2 * pad - K) // stride + 1, (Wi + 2 * pad - K) // stride + 1
    xb = torch.full((N, Hi, Wi, xcs), float("nan"))
    xb[..., xcoff:xcoff + cin] = x
    xb = xb.cuda()
    y = torch.full((N, Ho, Wo, ycs), float("nan"), device="cuda")
    hip.check(hip.lib().ssr_conv_direct(hip.View(xb.data_ptr(), xcs, xcoff), hip.View(y.data_ptr(), ycs, ycoff), wd.data_ptr(),
                                        bias.data_ptr() if bias is not None else None, hip.F32, N, Hi, Wi, cin, cout, K, stride, pad,
                                        relu, hip.stream_ptr()), "ssr_conv_direct")
    return y.cpu().numpy()


@pytest.mark.parametrize("epilogue", ["bias+relu", "plain"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_direct_matches_float64(case, epilogue):
    """Bound per output, for ANY fp32 summation order with or without fused multiply-add:
        |err| <= gamma_(K+1) (sum_i |x_i w_i| + |b|) + K 2^-126,   gamma_n = n u / (1 - n u), u = 2^-24, K = KH KW Cin
    (K products and the bias, one rounding each at the most; the last term covers products a subnormal-flushing matrix core drops).
    With the ReLU the bound holds unchanged (max(0, .) is 1-Lipschitz).  Nothing here comes from what the kernel returns.
    Input and output are channel slices of wider buffers whose other channels are NaN: none is read, none is written."""
    name, K, stride, pad, cin_v, cin, cout, N, Hi, Wi = case
    relu = 1 if epilogue == "bias+relu" else 0
    g = torch.Generator().manual_seed(1000 * K + 10 * Hi + Wi + relu)
    x = torch.zeros(N, Hi, Wi, cin)
    x[..., :cin_v] = torch.randn(N, Hi, Wi, cin_v, generator=g)          # (conv1: the 5 padding channels are 0, as ssr_lpips_input writes them)
    w = torch.randn(cout, cin_v, K, K, generator=g) / (K * K * cin_v) ** 0.5
    b = torch.randn(cout, generator=g) if relu else None
    wd = torch.zeros(K * K, cin, cout)
    wd[:, :cin_v] = w.permute(2, 3, 1, 0).reshape(K * K, cin_v, cout)
    wd, bd = wd.cuda(), (b.cuda() if relu else None)
    x64 = x[..., :cin_v].permute(0, 3, 1, 2).double()
    want = F.conv2d(x64, w.double(), b.double() if relu else None, stride=stride, padding=pad)
    mag = F.conv2d(x64.abs(), w.double().abs(), b.double().abs() if relu else None, stride=stride, padding=pad)
    if relu:
        want = want.clamp_min(0)
    want, mag = want.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()
    Kn = K * K * cin
    gamma = (Kn + 1) * U32 / (1 - (Kn + 1) * U32)
    tol = gamma * mag + Kn * 2.0 ** -126
    xcs, xcoff, ycs, ycoff = cin + 8, 4, cout + 16, 8
    geo = (cin, cout, K, stride, pad, relu, xcs, xcoff, ycs, ycoff)
    y1 = _conv_direct(x, wd, bd, N, Hi, Wi, *geo)
    y2 = _conv_direct(x, wd, bd, N, Hi, Wi, *geo)
    assert y1.shape[:3] == want.shape[:3]
    got = y1[..., ycoff:ycoff + cout]
    assert not np.isnan(got).any()                                         # every output written, nothing outside the Cin channels read
    assert np.isnan(np.delete(y1, np.s_[ycoff:ycoff + cout], axis=-1)).all()   # channels outside the output slice untouched
    assert y1.tobytes() == y2.tobytes()                                    # a second launch: the same bytes
    one = _conv_direct(x[:1], wd, bd, 1, Hi, Wi, *geo)
    assert one.tobytes() == y1[:1].tobytes()                               # image 0 alone: the same bytes as in the batch
    err = np.abs(got.astype(np.float64) - want)
    print(f"conv_direct {name} {epilogue}: max |err| {err.max():.3e}, max err / bound {np.max(err / tol):.3f}, max |y| {np.abs(want).max():.3f}")
    assert (err <= tol).all(), (float(err.max()), float(np.max(err / tol)))
    if relu:
        assert (got >= 0).all() and (got == 0).any()


def test_conv_direct_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    x = torch.zeros(1, 5, 5, 16, device="cuda")
    y = torch.full((1, 5, 5, 32), 7.0, device="cuda")
    w = torch.zeros(9, 16, 32, device="cuda")
    big = torch.zeros(1, 5, 5, 1024, device="cuda")

    def call(xv=hip.view(x), yv=hip.view(y), wp=w.data_ptr(), dt=hip.F32, N=1, Hi=5, Wi=5, cin=16, cout=32, K=3, s=1, p=1):
        return L.ssr_conv_direct(xv, yv, wp, None, dt, N, Hi, Wi, cin, cout, K, s, p, 0, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2
    assert call(K=4) == -2 and call(K=13) == -2 and call(s=5) == -2 and call(p=2) == -2
    assert call(cin=12) == -2 and call(cout=16) == -2
    assert call(xv=hip.view(big), cin=520) == -2 and call(yv=hip.view(big), cout=544) == -2
    assert call(xv=hip.NULL_VIEW) == -1 and call(yv=hip.NULL_VIEW) == -1 and call(wp=None) == -1
    assert call(N=0) == -1 and call(Hi=0) == -1 and call(Wi=0) == -1 and call(cin=0) == -1 and call(cout=0) == -1
    assert call(K=0) == -1 and call(s=0) == -1 and call(p=-1) == -1
    assert call(Hi=1, Wi=1, K=5, p=1) == -1                                      # no output pixel
    assert call(xv=hip.View(x.data_ptr(), 16, 8)) == -1                          # 8 + 16 channels do not fit a 16-channel view
    assert call(yv=hip.View(y.data_ptr(), 32, 4)) == -1
    assert call(xv=hip.View(x.data_ptr() + 4, 16, 0)) == -1                      # misaligned
    assert call(yv=hip.View(big.data_ptr(), 1024, 2)) == -1                      # coff % 4
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                                # no launch in any of these cases
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((y == 0.0).all())


# ------------------------------------------------------------------ ssr_maxpool3s2_fwd
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [64, 192])
@pytest.mark.parametrize("H,W", [(7, 7), (8, 11), (15, 15), (3, 3)])
def test_maxpool3s2_is_bit_exact(H, W, C, relu):
    """against F.max_pool2d(x, 3, 2) (of relu(x) with the flag): negatives, ties, -0.0 and +0.0 (compared after + 0.0), on a
    channel slice of a wider buffer on both sides"""
    from satlas_super_resolution_amd import hip
    g = torch.Generator().manual_seed(100 * H + W + C + relu)
    x = torch.randint(-3, 4, (2, H, W, C), generator=g).float() * 0.5           # few distinct values: ties in most windows
    x[torch.rand(2, H, W, C, generator=g) < 0.2] = -0.0
    x[0, 0, 0, :8] = torch.tensor([-0.0, 0.0, -1.5, 1.5, -0.0, 0.0, -0.5, 0.5])
    x[1] = x[1] - 2.0 * (torch.arange(C) % 2)                                   # odd channels of image 1: windows that are all negative
    xin = F.relu(x) if relu else x
    want = F.max_pool2d(xin.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    assert want.shape == (2, Ho, Wo, C)
    fcs, fcoff, pcs, pcoff = C + 8, 4, C + 12, 8
    fb = torch.full((2, H, W, fcs), float("nan"))
    fb[..., fcoff:fcoff + C] = x
    fb = fb.cuda()
    p = torch.full((2, Ho, Wo, pcs), float("nan"), device="cuda")
    hip.check(hip.lib().ssr_maxpool3s2_fwd(hip.View(fb.data_ptr(), fcs, fcoff), hip.View(p.data_ptr(), pcs, pcoff), hip.F32, 2, H, W, C,
                                           relu, hip.stream_ptr()), "ssr_maxpool3s2_fwd")
    got = p.cpu()
    assert bool(torch.isnan(torch.cat([got[..., :pcoff], got[..., pcoff + C:]], dim=-1)).all())
    a, b = (got[..., pcoff:pcoff + C] + 0.0).numpy(), (want + 0.0).numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_maxpool3s2_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    f = torch.zeros(1, 5, 5, 8, device="cuda")
    p = torch.full((1, 2, 2, 8), 7.0, device="cuda")

    def call(fv=hip.view(f), pv=hip.view(p), dt=hip.F32, N=1, H=5, W=5, C=8):
        return L.ssr_maxpool3s2_fwd(fv, pv, dt, N, H, W, C, 0, hip.stream_ptr())

    assert call(dt=hip.BF16) == -2 and call(C=6) == -2
    assert call(fv=hip.NULL_VIEW) == -1 and call(pv=hip.NULL_VIEW) == -1
    assert call(N=0) == -1 and call(C=0) == -1 and call(H=2) == -1 and call(W=2) == -1
    assert call(fv=hip.View(f.data_ptr(), 8, 4)) == -1 and call(pv=hip.View(p.data_ptr(), 4, 0)) == -1
    assert call(fv=hip.View(f.data_ptr() + 4, 8, 0)) == -1
    torch.cuda.synchronize()
    assert bool((p == 7.0).all())                                          # no launch in any of these cases
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((p == 0.0).all())


# ------------------------------------------------------------------ end to end
CASES = [(N, H, W, pair, cfg) for (N, H, W) in ((2, 31, 31), (1, 35, 47), (2, 64, 64)) for pair in ("independent", "noise8")
         for cfg in ("reference", "rgb+normalize")]
CFG = {"reference": dict(bgr=True, normalize=False), "rgb+normalize": dict(bgr=False, normalize=True)}


def _images(N, H, W, pair):
    g = torch.Generator().manual_seed(H * 131 + W + (7 if pair == "noise8" else 0))
    a = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    if pair == "independent":
        b = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    else:
        b = (a.int() + torch.randint(-8, 9, (N, H, W, 3), generator=g, dtype=torch.int32)).clamp(0, 255).to(torch.uint8)
    return a, b


@pytest.fixture(scope="module")
def lp():
    """the random network (non-zero biases), the CPU references of every end-to-end case (computed once) and the gate they give
    the device: 10 x the largest relative deviation of the float32 CPU evaluation from the float64 one over exactly these cases -
    one order of magnitude for a different summation order through five convolution layers"""
    from satlas_super_resolution_amd import lpips_metric as LM
    state = LM.lpips_random_state(17, net="alex")
    assert all(float(state[f"features.{i}.bias"].abs().min()) > 0 for i in (0, 3, 6, 8, 10))
    ref, cpu32 = {}, 0.0
    for case in CASES:
        N, H, W, pair, cfg = case
        a, b = _images(N, H, W, pair)
        r64 = LM.lpips_reference(a, b, state, dtype=torch.float64, net="alex", **CFG[cfg])
        r32 = LM.lpips_reference(a, b, state, dtype=torch.float32, net="alex", **CFG[cfg]).double()
        ref[case] = r64
        cpu32 = max(cpu32, float(((r32 - r64).abs() / r64).max()))
    print(f"lpips alex end to end: largest relative deviation of the float32 CPU evaluation from float64: {cpu32:.3e}; device gate {10 * cpu32:.3e}")
    return {"LM": LM, "state": state, "ref": ref, "cpu32": cpu32, "gate": 10 * cpu32, "model": LM.LPIPSModel(state, "cuda", net="alex")}


@pytest.mark.parametrize("N,H,W,pair,cfg", CASES)
def test_lpips_distance_matches_reference(lp, N, H, W, pair, cfg):
    """31 x 31: taps of 7, 3, 1, 1, 1 pixels a side.  The gate is the fixture's (10 x the float32 CPU deviation); the figures
    this printed on an MI355X are in profiles/lpips_alex/observed_errors.txt."""
    LM = lp["LM"]
    a, b = _images(N, H, W, pair)
    ad, bd = a.cuda(), b.cuda()
    want = lp["ref"][(N, H, W, pair, cfg)]
    got = LM.lpips_distance(ad, bd, lp["model"], **CFG[cfg])
    assert got.dtype == torch.float64 and got.shape == (N,) and not got.is_cuda
    rel = float(((got - want).abs() / want).max())
    print(f"lpips_distance alex {N}x{H}x{W} {pair} {cfg}: d = {want.tolist()}, device rel err {rel:.3e} (gate {lp['gate']:.3e})")
    again = LM.lpips_distance(ad, bd, lp["model"], **CFG[cfg])
    assert got.numpy().tobytes() == again.numpy().tobytes()
    assert torch.equal(LM.lpips_distance(ad, ad, lp["model"], **CFG[cfg]), torch.zeros(N, dtype=torch.float64))
    assert rel <= lp["gate"], (rel, lp["gate"])


def test_lpips_launch_list(lp):
    """the AlexNet plan: two inputs, conv1 and conv2 direct, two poolings, three 3x3 layers, five taps with relu = 0"""
    from satlas_super_resolution_amd import hip
    plan = lp["model"].plan(2, 64, 64)
    lib = hip.lib()
    fns = [fn for fn, _, _ in plan.launcher.flat_calls()]
    assert fns.count(lib.ssr_lpips_input) == 2 and fns.count(lib.ssr_maxpool3s2_fwd) == 2 and fns.count(lib.ssr_lpips_layer) == 5
    assert fns.count(lib.ssr_conv_direct) + fns.count(lib.ssr_conv2d) == 5 and fns.count(lib.ssr_conv_direct) >= 2
    assert len(fns) == 14
    assert all(args[7] == 0 for fn, args, _ in plan.launcher.flat_calls() if fn is lib.ssr_lpips_layer)


def test_lpips_distance_rejects_h30(lp):
    a = torch.zeros(1, 30, 40, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="30"):
        lp["LM"].lpips_distance(a, a, lp["model"])


# ------------------------------------------------------------------ through the model plugin
def test_calculate_lpips_through_the_test_pipeline(lp, tmp_path, monkeypatch):
    """`test.metrics = {psnr, lpips (alexnet), lpips_vgg (vgg)}` over the s2naip_mini set with weights files in the lpips package's
    combined layout: each logged value is the mean of lpips_reference of its backbone over the written PNG pairs (within the
    fixture's gate for AlexNet; VGG's own test holds its gate, here 1e-4 says it is the VGG number and not the other); both
    models sit in the cache at once; without the weights key the same option file raises before the first image."""
    from PIL import Image
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.test import test_pipeline
    LM, state = lp["LM"], lp["state"]
    monkeypatch.delenv("SSR_LPIPS_WEIGHTS", raising=False)
    monkeypatch.delenv("SSR_LPIPS_ALEX_WEIGHTS", raising=False)
    monkeypatch.chdir(tmp_path)                                       # no experiments/pretrained_models/lpips_alex.pth here
    head = {"scaling_layer.shift": torch.tensor(LM.LPIPS_SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(LM.LPIPS_SCALE).view(1, 3, 1, 1)}

    def combined(st, slices):
        sd = dict(head)
        for s, idxs in slices.items():
            for i in idxs:
                sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"] = st[f"features.{i}.weight"], st[f"features.{i}.bias"]
        for k in range(5):
            sd[f"lin{k}.model.1.weight"] = sd[f"lins.{k}.model.1.weight"] = st[f"lin{k}"].view(1, -1, 1, 1)
        return sd

    vstate = LM.lpips_random_state(17)
    torch.save(combined(state, {1: (0,), 2: (3,), 3: (6,), 4: (8,), 5: (10,)}), tmp_path / "lpips_alex.pth")
    torch.save(combined(vstate, {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}), tmp_path / "lpips_vgg.pth")
    mini = os.path.join(GOLDEN, "s2naip_mini")
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=1, num_grow_ch=32)
    gsd = O.generator_init(seed=5, **g_kw)
    torch.save({"params": gsd, "params_ema": gsd}, tmp_path / "net_g.pth")
    metrics = {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": False},
               "lpips": {"type": "calculate_lpips", "lpips_model": "alexnet", "better": "lower", "lpips_weights": str(tmp_path / "lpips_alex.pth")},
               "lpips_vgg": {"type": "calculate_lpips", "lpips_model": "vgg", "better": "lower", "lpips_weights": str(tmp_path / "lpips_vgg.pth")}}
    opt = {"name": "t", "model_type": "SSRESRGANModel", "scale": 4, "manual_seed": 0, "compute_dtype": "fp32x3",
           "test_datasets": {"test": {"name": "test", "type": "S2NAIPDataset", "phase": "test", "scale": 4, "n_s2_images": 8,
                                      "sentinel2_path": os.path.join(mini, "sentinel2"), "naip_path": os.path.join(mini, "naip")}},
           "network_g": dict(type="SSR_RRDBNet", **g_kw),
           "path": {"pretrain_network_g": str(tmp_path / "net_g.pth"), "param_key_g": "params_ema", "strict_load_g": True,
                    "visualization": str(tmp_path / "vis")},
           "test": {"save_img": True, "metrics": metrics}}
    res = test_pipeline(opt, log=lambda *_: None)
    assert set(res) == {"test"} and set(res["test"]) == {"psnr", "lpips", "lpips_vgg"}
    load = lambda f: torch.from_numpy(np.asarray(Image.open(tmp_path / "vis" / "test" / f)).copy())[None]        # noqa: E731
    sr = torch.cat([load(f"{i}_t.png") for i in range(5)])
    gt = torch.cat([load(f"{i}_t_gt.png") for i in range(5)])
    assert sr.shape == gt.shape == (5, 128, 128, 3)
    want = float(LM.lpips_reference(sr, gt, state, net="alex").mean())
    rel = abs(res["test"]["lpips"] - want) / want
    print(f"calculate_lpips (alexnet) through the test pipeline: {res['test']['lpips']!r} against {want!r}: rel err {rel:.3e} (gate {lp['gate']:.3e})")
    assert want > 0 and rel <= lp["gate"]
    want_v = float(LM.lpips_reference(sr, gt, vstate).mean())
    rel_v = abs(res["test"]["lpips_vgg"] - want_v) / want_v
    print(f"calculate_lpips (vgg) in the same run: {res['test']['lpips_vgg']!r} against {want_v!r}: rel err {rel_v:.3e}")
    assert want_v > 0 and rel_v <= 1e-4 and abs(want_v - want) / want > 1e-2
    nets = sorted(k[0] for k in LM._MODELS if k[1] in (str((tmp_path / "lpips_alex.pth").resolve()), str((tmp_path / "lpips_vgg.pth").resolve())))
    assert nets == ["alex", "vgg"]
    bad = dict(opt, test={"save_img": False, "metrics": {"lpips": {"type": "calculate_lpips", "lpips_model": "alexnet"}}})
    with pytest.raises(NotImplementedError, match="lpips_model='alexnet'"):
        test_pipeline(bad, log=lambda *_: None)
