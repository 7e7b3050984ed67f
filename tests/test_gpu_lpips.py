"""GPU: the LPIPS metric on the device (lpips_metric.py + csrc/lpips.hip + the exact-fp32 convolutions) against the CPU
statement of its definition (lpips_metric.lpips_reference, float64): the two C-ABI entries on their own, the whole metric
through lpips_distance, and `calculate_lpips` through the model plugin's test pipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53


# ------------------------------------------------------------------ ssr_lpips_input
@pytest.mark.parametrize("bgr,normalize", [(True, False), (True, True), (False, False), (False, True)])
def test_lpips_input_is_bit_exact(bgr, normalize):
    """N = 2 images of 4 x 6 pixels against numpy float32 in the order include/ssr_hip.h states; padding channels 0; a view
    with cs > coff + 8 keeps its other channels."""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.lpips_metric import LPIPS_SCALE, LPIPS_SHIFT
    rng = np.random.default_rng(5)
    u = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    u[0, 0, 0] = (0, 255, 128)
    shift, scale = np.asarray(LPIPS_SHIFT, np.float32), np.asarray(LPIPS_SCALE, np.float32)
    perm = (2, 1, 0) if bgr else (0, 1, 2)
    v = u[..., list(perm)].astype(np.float32) / np.float32(255.0)
    if normalize:
        v = np.float32(2.0) * v - np.float32(1.0)
    want = (v - shift) / scale
    assert want.dtype == np.float32
    ud = torch.from_numpy(u).cuda()
    args = ((ctypes.c_float * 3)(*shift.tolist()), (ctypes.c_float * 3)(*scale.tolist()), (ctypes.c_int32 * 3)(*perm), 1 if normalize else 0)
    for cs, coff in ((8, 0), (16, 4)):
        y = torch.full((2, 4, 6, cs), float("nan"), device="cuda")
        hip.check(hip.lib().ssr_lpips_input(ud.data_ptr(), hip.View(y.data_ptr(), cs, coff), hip.F32, 2 * 4 * 6, *args, hip.stream_ptr()),
                  "ssr_lpips_input")
        got = y.cpu().numpy()
        assert np.array_equal(got[..., coff:coff + 3].view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got[..., coff + 3:coff + 8], np.zeros((2, 4, 6, 5), np.float32))
        rest = np.delete(got, np.s_[coff:coff + 8], axis=-1)
        assert np.isnan(rest).all()


def test_lpips_input_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    u = torch.zeros(24, 3, dtype=torch.uint8, device="cuda")
    y = torch.full((24, 8), 7.0, device="cuda")
    sh, sc, pm = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int32 * 3)(0, 1, 2)
    ok = lambda **k: L.ssr_lpips_input(k.get("u", u.data_ptr()), k.get("y", hip.view(y)), k.get("dt", hip.F32), k.get("n", 24), sh,     # noqa: E731
                                       k.get("sc", sc), k.get("pm", pm), 0, hip.stream_ptr())
    assert ok(dt=hip.BF16) == -2
    assert ok(u=None) == -1 and ok(y=hip.NULL_VIEW) == -1 and ok(n=0) == -1
    assert ok(y=hip.View(y.data_ptr(), 8, 4)) == -1                        # narrower than coff + 8
    assert ok(pm=(ctypes.c_int32 * 3)(0, 1, 3)) == -1 and ok(sc=(ctypes.c_float * 3)(1, 0, 1)) == -1
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                          # no launch in any of these cases
    assert ok() == 0


# ------------------------------------------------------------------ ssr_lpips_layer
def _layer_reference(a, b, w, relu):
    """float64 numpy on the fp32 inputs -> (d[N], tol[N]); the bound is derived in test_lpips_layer_matches_float64"""
    a, b, w = a.astype(np.float64), b.astype(np.float64), w.astype(np.float64)
    if relu:
        a, b = np.maximum(a, 0), np.maximum(b, 0)
    C = a.shape[-1]
    ah = a / (np.sqrt((a * a).sum(-1, keepdims=True)) + 1e-10)
    bh = b / (np.sqrt((b * b).sum(-1, keepdims=True)) + 1e-10)
    d = ah - bh
    t = w * d * d
    hw = a.shape[1]
    delta = 2 * (C + 8) * U64 * (np.abs(ah) + np.abs(bh))
    per_term = 4.5 * U32 * t + w * (2 * np.abs(d) * delta + delta * delta) + w * 1e-37
    tol = per_term.sum((1, 2)) / hw + 2 * (C * hw + 300) * U64 * t.sum((1, 2)) / hw
    return t.sum((1, 2)) / hw, tol


def _layer_run(fa, fb, w, N, HW, C, relu, cs, coff):
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    nblk = L.ssr_lpips_layer_blocks(N, HW, C)
    assert nblk >= 1
    part = torch.full((N, nblk), float("nan"), dtype=torch.float64, device="cuda")
    hip.check(L.ssr_lpips_layer(hip.View(fa.data_ptr(), cs, coff), hip.View(fb.data_ptr(), cs, coff), w.data_ptr(), hip.F32, N, HW, C,
                                relu, part.data_ptr(), hip.stream_ptr()), "ssr_lpips_layer")
    return part.cpu().numpy()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N,HW,C", [(2, 256, 64), (2, 15, 64), (1, 1, 512), (1, 3, 512), (2, 64, 128), (1, 16, 256)])
def test_lpips_layer_matches_float64(N, HW, C, relu):
    """The partials of one tap, added in index order, against float64 numpy on the same fp32 inputs.

    Bound, per term t = w (a^ - b^)^2 with u = 2^-24 (fp32) and v = 2^-53 (fp64), from the arithmetic include/ssr_hip.h states:
      * the norms are fp64 sums of exact squares, C + 3 additions, a square root, an addition and a reciprocal: each normalised
        value carries a relative error below (C + 8) v, so the difference d carries an ABSOLUTE error below
        delta = (C + 8) v (|a^| + |b^|); the float64 reference carries as much, hence 2 delta: t moves by w (2 |d| delta + delta^2);
      * d is rounded to fp32 (u), d * d squares that and rounds (2 u + u), w * (d * d) rounds once more (u): 4 u relative, taken
        as 4.5 u for the second-order terms; a product that underflows fp32 (|d| < 1e-19) loses at most w * 1e-37;
      * the fp64 sum of the C * HW terms (and of at most 256 partials on the host) moves the total by below (C HW + 300) v
        relative, in the device's and in the reference's order.
    Nothing here comes from what the kernel returns.  Inputs have negative values, one pixel whose channels are all <= 0 (zero
    norm behind the ReLU) and sit in a view with cs > C, coff > 0 whose other channels are NaN."""
    rng = np.random.default_rng(1000 * C + 10 * HW + relu)
    a = rng.standard_normal((N, HW, C)).astype(np.float32)
    b = (a + 0.25 * rng.standard_normal((N, HW, C))).astype(np.float32) if HW % 2 else rng.standard_normal((N, HW, C)).astype(np.float32)
    a[0, 0] = -np.abs(a[0, 0])
    a[0, 0, ::2] = 0.0
    w = rng.random(C).astype(np.float32)
    cs, coff = C + 16, 8

    def dev(x):
        buf = torch.full((N, HW, cs), float("nan"))
        buf[..., coff:coff + C] = torch.from_numpy(x)
        return buf.cuda()

    fa, fb, wd = dev(a), dev(b), torch.from_numpy(w).cuda()
    want, tol = _layer_reference(a, b, w, relu)
    p1 = _layer_run(fa, fb, wd, N, HW, C, relu, cs, coff)
    p2 = _layer_run(fa, fb, wd, N, HW, C, relu, cs, coff)
    assert not np.isnan(p1).any()                              # every partial written, nothing outside the C channels read
    assert p1.tobytes() == p2.tobytes()
    got = p1.cumsum(axis=1)[:, -1]
    err = np.abs(got - want)
    print(f"lpips_layer N={N} HW={HW} C={C} relu={relu}: rel err {np.max(err / want):.3e}, bound {np.max(tol / want):.3e}")
    assert (want > 0).all() and (err <= tol).all(), (got, want, err, tol)
    same = _layer_run(fa, fa, wd, N, HW, C, relu, cs, coff)
    assert np.array_equal(same, np.zeros_like(same))           # exactly 0.0, every partial


def test_lpips_layer_error_codes():
    from satlas_super_resolution_amd import hip
    L = hip.lib()
    f = torch.zeros(1, 4, 128, device="cuda")
    w = torch.zeros(128, device="cuda")
    part = torch.full((4,), 3.0, dtype=torch.float64, device="cuda")
    v = hip.view(f)
    call = lambda fa=v, fb=v, wp=w.data_ptr(), dt=hip.F32, N=1, HW=4, C=128, pp=part.data_ptr(): \
        L.ssr_lpips_layer(fa, fb, wp, dt, N, HW, C, 1, pp, hip.stream_ptr())                               # noqa: E731
    assert call(dt=hip.BF16) == -2
    assert call(C=96) == -2
    assert call(fa=hip.NULL_VIEW) == -1 and call(fb=hip.NULL_VIEW) == -1 and call(wp=None) == -1 and call(pp=None) == -1
    assert call(N=0) == -1 and call(HW=0) == -1 and call(C=0) == -1
    assert call(fa=hip.View(f.data_ptr(), 128, 64)) == -1                 # 64 + 128 channels do not fit a 128-channel view
    assert call(fb=hip.View(f.data_ptr(), 64, 0)) == -1
    assert L.ssr_lpips_layer_blocks(0, 4, 128) == -1 and L.ssr_lpips_layer_blocks(1, 4, 128) >= 1
    torch.cuda.synchronize()
    assert bool((part == 3.0).all())                                       # no launch in any of these cases
    assert call() == 0


# ------------------------------------------------------------------ end to end
CASES = [(N, H, W, pair, cfg) for (N, H, W) in ((2, 32, 32), (1, 16, 48)) for pair in ("independent", "noise8")
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
    """the random network, the CPU references of every end-to-end case (computed once) and the gate they give the device:
    10 x the largest relative deviation of the float32 CPU evaluation from the float64 one over exactly these cases - one order
    of magnitude for a different summation order through 13 convolution layers"""
    from satlas_super_resolution_amd import lpips_metric as LM
    state = LM.lpips_random_state(17)
    ref, cpu32 = {}, 0.0
    for case in CASES:
        N, H, W, pair, cfg = case
        a, b = _images(N, H, W, pair)
        r64 = LM.lpips_reference(a, b, state, dtype=torch.float64, **CFG[cfg])
        r32 = LM.lpips_reference(a, b, state, dtype=torch.float32, **CFG[cfg]).double()
        ref[case] = r64
        cpu32 = max(cpu32, float(((r32 - r64).abs() / r64).max()))
    print(f"lpips end to end: largest relative deviation of the float32 CPU evaluation from float64: {cpu32:.3e}; device gate {10 * cpu32:.3e}")
    return {"LM": LM, "state": state, "ref": ref, "cpu32": cpu32, "gate": 10 * cpu32, "model": LM.LPIPSModel(state, "cuda")}


@pytest.mark.parametrize("N,H,W,pair,cfg", CASES)
def test_lpips_distance_matches_reference(lp, N, H, W, pair, cfg):
    """16 x 48: the last tap is 1 x 3 pixels.  The gate is the fixture's (10 x the float32 CPU deviation); the figures this
    printed on an MI355X are in profiles/lpips_metric/observed_errors.txt."""
    LM = lp["LM"]
    a, b = _images(N, H, W, pair)
    ad, bd = a.cuda(), b.cuda()
    want = lp["ref"][(N, H, W, pair, cfg)]
    got = LM.lpips_distance(ad, bd, lp["model"], **CFG[cfg])
    assert got.dtype == torch.float64 and got.shape == (N,) and not got.is_cuda
    rel = float(((got - want).abs() / want).max())
    print(f"lpips_distance {N}x{H}x{W} {pair} {cfg}: d = {want.tolist()}, device rel err {rel:.3e} (gate {lp['gate']:.3e})")
    again = LM.lpips_distance(ad, bd, lp["model"], **CFG[cfg])
    assert got.numpy().tobytes() == again.numpy().tobytes()
    assert torch.equal(LM.lpips_distance(ad, ad, lp["model"], **CFG[cfg]), torch.zeros(N, dtype=torch.float64))
    assert rel <= lp["gate"], (rel, lp["gate"])


def test_lpips_distance_rejects_h24(lp):
    a = torch.zeros(1, 24, 32, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="24"):
        lp["LM"].lpips_distance(a, a, lp["model"])


# ------------------------------------------------------------------ through the model plugin
def test_calculate_lpips_through_the_test_pipeline(lp, tmp_path, monkeypatch):
    """`test.metrics = {psnr, lpips}` over the s2naip_mini set with a weights file in the lpips package's combined layout: the
    logged value is the mean of lpips_reference over the written PNG pairs (within the fixture's gate); without the weights key
    the same option file raises before the first image."""
    from PIL import Image
    from oracle import esrgan_oracle as O
    from satlas_super_resolution_amd.test import test_pipeline
    LM, state = lp["LM"], lp["state"]
    monkeypatch.delenv("SSR_LPIPS_WEIGHTS", raising=False)
    slices = {1: (0, 2), 2: (5, 7), 3: (10, 12, 14), 4: (17, 19, 21), 5: (24, 26, 28)}
    sd = {"scaling_layer.shift": torch.tensor(LM.LPIPS_SHIFT).view(1, 3, 1, 1), "scaling_layer.scale": torch.tensor(LM.LPIPS_SCALE).view(1, 3, 1, 1)}
    for s, idxs in slices.items():
        for i in idxs:
            sd[f"net.slice{s}.{i}.weight"], sd[f"net.slice{s}.{i}.bias"] = state[f"features.{i}.weight"], state[f"features.{i}.bias"]
    for k in range(5):
        sd[f"lin{k}.model.1.weight"] = sd[f"lins.{k}.model.1.weight"] = state[f"lin{k}"].view(1, -1, 1, 1)
    torch.save(sd, tmp_path / "lpips_vgg.pth")
    mini = os.path.join(GOLDEN, "s2naip_mini")
    g_kw = dict(num_in_ch=24, num_out_ch=3, scale=4, num_feat=64, num_block=1, num_grow_ch=32)
    gsd = O.generator_init(seed=5, **g_kw)
    torch.save({"params": gsd, "params_ema": gsd}, tmp_path / "net_g.pth")
    metrics = {"psnr": {"type": "calculate_psnr", "crop_border": 4, "test_y_channel": False},
               "lpips": {"type": "calculate_lpips", "lpips_model": "vgg", "better": "lower", "lpips_weights": str(tmp_path / "lpips_vgg.pth")}}
    opt = {"name": "t", "model_type": "SSRESRGANModel", "scale": 4, "manual_seed": 0, "compute_dtype": "fp32x3",
           "test_datasets": {"test": {"name": "test", "type": "S2NAIPDataset", "phase": "test", "scale": 4, "n_s2_images": 8,
                                      "sentinel2_path": os.path.join(mini, "sentinel2"), "naip_path": os.path.join(mini, "naip")}},
           "network_g": dict(type="SSR_RRDBNet", **g_kw),
           "path": {"pretrain_network_g": str(tmp_path / "net_g.pth"), "param_key_g": "params_ema", "strict_load_g": True,
                    "visualization": str(tmp_path / "vis")},
           "test": {"save_img": True, "metrics": metrics}}
    res = test_pipeline(opt, log=lambda *_: None)
    assert set(res) == {"test"} and set(res["test"]) == {"psnr", "lpips"}
    load = lambda f: torch.from_numpy(np.asarray(Image.open(tmp_path / "vis" / "test" / f)).copy())[None]        # noqa: E731
    sr = torch.cat([load(f"{i}_t.png") for i in range(5)])
    gt = torch.cat([load(f"{i}_t_gt.png") for i in range(5)])
    assert sr.shape == gt.shape == (5, 128, 128, 3)
    want = float(LM.lpips_reference(sr, gt, state).mean())
    rel = abs(res["test"]["lpips"] - want) / want
    print(f"calculate_lpips through the test pipeline: {res['test']['lpips']!r} against {want!r}: rel err {rel:.3e} (gate {lp['gate']:.3e})")
    assert want > 0 and rel <= lp["gate"]
    bad = dict(opt, test={"save_img": False, "metrics": {"lpips": {"type": "calculate_lpips", "lpips_model": "vgg"}}})
    with pytest.raises(NotImplementedError, match="calculate_lpips"):
        test_pipeline(bad, log=lambda *_: None)
