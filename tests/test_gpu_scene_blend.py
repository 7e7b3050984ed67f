"""GPU: blended scene inference (satlas_super_resolution_amd/infer_scene.py, csrc/scene.hip) - the four kernels for chunks at
arbitrary places against numpy and `blend_reference` of tests/test_scene_blend_host.py, `super_resolve_scene_blended` against the same
chunks through the module's forward and that restatement, and the driver's `overlap:` option.  Every comparison is exact.
Fixture-sized generators only (num_feat 16, num_block 1)."""
import os
import random

import numpy as np
import pytest
import torch
import yaml

from test_scene_blend_host import blend_accumulate, blend_finish, blend_reference, grid_of

pytestmark = pytest.mark.gpu


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB")).copy()


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def _inside(y0, x0, H, W):
    return 0 <= y0 <= H - 32 and 0 <= x0 <= W - 32


# ---------------------------------------------------------------- 1. zero scan and gather at odd places
H1, W1 = 49, 50                                   # a row of the scene is 150 bytes: rows and windows start at every alignment
ORIGINS1 = [(0, 0), (17, 18), (7, 13), (18, 3), (3, 1), (16, 17), (5, 19), (-1, 4)]     # (18, 3), (5, 19), (-1, 4): outside


def test_zero_scan_at_odd_origins_finds_planted_zeros_and_nothing_else():
    from satlas_super_resolution_amd import hip
    rng = np.random.RandomState(12)
    T = 3
    scene = rng.randint(1, 256, size=(T, H1, W1, 3)).astype(np.uint8)
    # the first and the last byte of the scene; the last byte of the window at (7, 13) and the byte right of its first row; the byte
    # left of the last row of the window at (17, 18); the first byte of the window at (16, 17)
    for t, y, x, c in [(0, 0, 0, 0), (2, 48, 49, 2), (1, 38, 44, 2), (1, 7, 45, 0), (0, 48, 17, 2), (2, 16, 17, 0)]:
        scene[t, y, x, c] = 0
    want = np.full((len(ORIGINS1), T), 7, np.uint8)
    for b, (y0, x0) in enumerate(ORIGINS1):
        if _inside(y0, x0, H1, W1):
            want[b] = (scene[:, y0:y0 + 32, x0:x0 + 32] == 0).any(axis=(1, 2, 3))
    assert (want == 0).any() and (want == 1).any()
    dev_scene = torch.from_numpy(scene).cuda()
    origins = torch.tensor(ORIGINS1, dtype=torch.int32, device="cuda")
    got = torch.full((len(ORIGINS1), T), 7, dtype=torch.uint8, device="cuda")       # an item outside the scene keeps the 7s
    hip.check(hip.lib().ssr_scene_zero_scan_at(dev_scene.data_ptr(), T, H1, W1, origins.data_ptr(), len(ORIGINS1), got.data_ptr(),
                                               hip.stream_ptr()), "ssr_scene_zero_scan_at")
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    from satlas_super_resolution_amd.infer_scene import scene_zero_scan_at
    ok = [b for b, o in enumerate(ORIGINS1) if _inside(*o, H1, W1)]
    assert np.array_equal(scene_zero_scan_at(dev_scene, origins[ok].contiguous()).cpu().numpy(), want[ok])
    # a scene whose base is not even 2-byte aligned: a view one byte into a larger buffer
    big = torch.zeros(scene.size + 1, dtype=torch.uint8, device="cuda")
    big[1:] = dev_scene.reshape(-1)
    shifted = big[1:].view(T, H1, W1, 3)
    assert shifted.data_ptr() % 2 == 1
    assert np.array_equal(scene_zero_scan_at(shifted, origins[ok].contiguous()).cpu().numpy(), want[ok])


# T = 3 with n = 1 and 3 (3 and 9 channels: element stores); 12 fp32 / 24 bf16 channels take the 16-byte stores and need T >= n
@pytest.mark.parametrize("storage,T,n,cs", [("fp32", 3, 1, 8), ("fp32", 3, 3, 16), ("bf16", 3, 1, 8), ("bf16", 3, 3, 16),
                                            ("fp32", 8, 4, 16), ("bf16", 8, 8, 24), ("bf16", 8, 8, 32)])
def test_gather_at_odd_origins_equals_frames_to_input_and_the_layout_converter(storage, T, n, cs):
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import scene_gather_at
    from satlas_super_resolution_amd.utils.infer_utils import frames_to_input
    rng = np.random.RandomState(6)
    scene = rng.randint(0, 256, size=(T, H1, W1, 3)).astype(np.uint8)
    assert len(np.unique(scene)) == 256                                  # every byte value goes through the conversion
    B = len(ORIGINS1)
    frame_ids = np.stack([rng.permutation(T)[:n] for _ in range(B)]).astype(np.int32)
    ok = np.array([_inside(y0, x0, H1, W1) for y0, x0 in ORIGINS1])
    sel = np.zeros((B, n, 32, 32, 3), np.uint8)
    for b, (y0, x0) in enumerate(ORIGINS1):
        if ok[b]:
            sel[b] = scene[frame_ids[b], y0:y0 + 32, x0:x0 + 32]
    dt = hip.dtype_code(storage)
    tdt = hip.torch_dtype(dt)
    x = frames_to_input(torch.from_numpy(sel).cuda()).contiguous()
    want = torch.full((B, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    hip.check(hip.lib().ssr_nchw_to_nhwc(x.data_ptr(), B, 3 * n, 32, 32, hip.view(want), dt, 1, 1, 1.0, hip.stream_ptr()), "ssr_nchw_to_nhwc")
    want[torch.from_numpy(~ok).cuda()] = -7.0                            # items outside the scene leave their destination as it was
    got = torch.full((B, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    big = torch.zeros(scene.size + 3, dtype=torch.uint8, device="cuda")  # the scene 3 bytes into a buffer: an odd base address
    big[3:] = torch.from_numpy(scene).cuda().reshape(-1)
    scene_gather_at(big[3:].view(T, H1, W1, 3), torch.tensor(ORIGINS1, dtype=torch.int32, device="cuda"),
                    torch.from_numpy(frame_ids).cuda(), got, dt)
    torch.cuda.synchronize()
    print(f"[{storage}, n = {n}, cs = {cs}] differing elements {int((got != want).sum())} of {got.numel()}")
    assert torch.equal(got, want)
    assert bool((got[..., 3 * n:] == -7.0).all()) and float(got[ok.tolist().index(True), ..., :3 * n].float().min()) >= 0.0


# ---------------------------------------------------------------- 2. blend-add and finish against blend_reference
def _synthetic_outputs(N, C, cs, seed):
    """[N, 128, 128, cs] fp32: values below 0 and above 1, exactly 0 and 1, multiples of 1/255 and their neighbours, a NaN, a +Inf and
    a -Inf among the C output channels (3 non-finite samples) and a NaN in a pad channel, which is no output sample"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.rand(N, 128, 128, cs, generator=g) * 1.6 - 0.3
    k = torch.randint(0, 256, (N, 128, 16, cs), generator=g).float() / 255
    buf[:, :, :16] = k
    buf[:, :, 16:32] = torch.where(torch.rand(k.shape, generator=g) < 0.5, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-1.0)))
    buf[:, 7, 40:50] = 0.0
    buf[:, 9, 40:50] = 1.0
    buf[0, 100, 100, 1] = float("nan")
    buf[N - 1, 127, 127, C - 1] = float("inf")
    buf[N // 2, 0, 0, 0] = float("-inf")
    buf[1, 64, 3, C] = float("nan")
    return buf, 3


def _blend_on_device(src, origins, order, splits, C, H, W, overlap, dt):
    """the items in `order`, cut into launches at `splits` -> (accumulator uint32 [4H, 4W, C], counter, mosaic) as numpy"""
    from satlas_super_resolution_amd.infer_scene import blend_weight_sums, blend_window, scene_blend_add, scene_blend_finish
    acc = torch.zeros(4 * H, 4 * W, C, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    window = torch.from_numpy(blend_window(overlap)).cuda()
    org = torch.tensor([origins[i] for i in order], dtype=torch.int32, device="cuda")
    s = src[list(order)].contiguous()
    bounds = [0] + list(splits) + [len(order)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        scene_blend_add(s[a:b], org[a:b].contiguous(), C, window, acc, counter, dt)
    mosaic = torch.full((4 * H, 4 * W, C), 9, dtype=torch.uint8, device="cuda")
    scene_blend_finish(acc, torch.from_numpy(blend_weight_sums(H, overlap)).cuda(), torch.from_numpy(blend_weight_sums(W, overlap)).cuda(), mosaic)
    torch.cuda.synchronize()
    return acc.cpu().numpy().view(np.uint32), int(counter[0]), mosaic.cpu().numpy()


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W,overlap", [(49, 50, 16), (40, 72, 8), (64, 96, 0)])
def test_blend_add_and_finish_equal_the_numpy_restatement_in_any_order_and_grouping(storage, H, W, overlap):
    from satlas_super_resolution_amd import hip
    C, cs = 3, 8
    origins = grid_of(H, W, overlap)
    N = len(origins)
    assert N == {(49, 50): 9, (40, 72): 6, (64, 96): 6}[(H, W)]
    origins = origins + [(H - 31, 0)]                                    # one item outside the scene: adds nothing, counts nothing
    buf, planted = _synthetic_outputs(N + 1, C, cs, seed=H)
    buf[N, 5, 5, 0] = float("nan")                                       # (in the skipped item)
    buf[N - 1, 127, 127, C - 1] = float("inf")                           # (_synthetic_outputs put it into the skipped item)
    dt = hip.dtype_code(storage)
    src = buf.to(hip.torch_dtype(dt)).cuda().contiguous()
    outs = src[..., :C].float().cpu().numpy()                            # the stored values, widened exactly
    want_acc = blend_accumulate(outs, origins, H, W, overlap)
    want = blend_finish(want_acc, H, W, overlap)
    assert np.array_equal(want, blend_reference(outs, origins, H, W, overlap))
    fwd = list(range(N))
    results = [_blend_on_device(src, origins, fwd, [], C, H, W, overlap, dt),            # one launch
               _blend_on_device(src, origins, fwd[::-1], [], C, H, W, overlap, dt),      # reversed
               _blend_on_device(src, origins, fwd, [4], C, H, W, overlap, dt),           # two launches: 4 + the rest (5 of the 9)
               _blend_on_device(src, origins, [N] + fwd, [], C, H, W, overlap, dt)]      # with the item outside the scene
    for acc, bad, mosaic in results:
        print(f"[{storage} {H} x {W} overlap {overlap}] differing accumulator words {int((acc != want_acc).sum())}, "
              f"differing bytes {int((mosaic != want).sum())} of {want.size}, counter {bad}")
        assert bad == planted
        assert np.array_equal(acc, want_acc)
        assert np.array_equal(mosaic, want)
    assert len(np.unique(want)) > 200


def test_the_largest_accumulator_value_every_sample_one_under_nine_fold_cover():
    from satlas_super_resolution_amd import hip
    H, W, overlap, C = 49, 50, 16, 3
    origins = grid_of(H, W, overlap)
    src = torch.ones(9, 128, 128, 8, device="cuda")
    want_acc = blend_accumulate(np.ones((9, 128, 128, C), np.float32), origins, H, W, overlap)
    acc, bad, mosaic = _blend_on_device(src, origins, range(9), [], C, H, W, overlap, hip.dtype_code("fp32"))
    print(f"largest accumulator word {int(want_acc.max())} = {int(want_acc.max()) / 2 ** 32:.3f} x 2^32")
    assert int(want_acc.max()) > 2 ** 29 and bad == 0
    assert np.array_equal(acc, want_acc)
    assert (mosaic == 255).all()


# ---------------------------------------------------------------- 3. end to end
def _small_model(n, compute_dtype="fp32h"):
    from oracle import esrgan_oracle as O
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    sd = O.generator_init(num_in_ch=3 * n, num_out_ch=3, scale=4, seed=M.SEED, **M.G_KW)
    sd["conv_last.bias"] = torch.full_like(sd["conv_last.bias"], 0.45)
    sd["conv_last.weight"] = sd["conv_last.weight"] * 8
    net = SSR_RRDBNet(num_in_ch=3 * n, num_out_ch=3, compute_dtype=compute_dtype, **M.G_KW)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval().freeze_packed()


def test_blended_scene_is_the_modules_chunks_through_the_numpy_restatement():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene_blended
    from satlas_super_resolution_amd.utils.infer_utils import frames_to_input, select_frames
    rng = np.random.RandomState(22)
    T, H, W, n, batch, overlap = 4, 40, 72, 2, 4, 8
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    scene = np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 255).astype(np.uint8)
    origins = grid_of(H, W, overlap)
    assert origins == [(0, 0), (0, 24), (0, 40), (8, 0), (8, 24), (8, 40)]
    scene[0, 3, 5, 1] = 0                          # in the chunks at (0, 0) only: one zero-holding frame
    scene[1, 39, 70, 0] = scene[2, 38, 71, 2] = scene[3, 39, 71, 2] = 0          # chunk (8, 40) only: one clean frame, topped up
    scene[:, 20, 30, 0] = 0                        # chunks (0, 0), (0, 24), (8, 0), (8, 24): every frame holds a zero
    model = _small_model(n)
    random.seed(5)
    got = super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    got = got.copy()
    # select_frames chunk by chunk in row-major order, the same batch grouping (a full batch and a ragged one)
    random.seed(5)
    sels = [select_frames(scene[:, y0:y0 + 32, x0:x0 + 32].reshape(T * 32, 32, 3), n)[0] for y0, x0 in origins]
    outs = []
    with torch.no_grad():
        for c0 in range(0, len(sels), batch):
            x = frames_to_input(torch.from_numpy(np.stack(sels[c0:c0 + batch])).cuda())
            outs.append(model(x).float().permute(0, 2, 3, 1).cpu().numpy())
    want = blend_reference(np.concatenate(outs), origins, H, W, overlap)
    print(f"differing bytes {int((got != want).sum())} of {want.size}")
    assert np.array_equal(got, want)
    assert float(got.std()) > 5
    random.seed(5)
    assert np.array_equal(super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch), got)      # same bytes again
    random.seed(5)
    assert np.array_equal(super_resolve_scene_blended(model, torch.from_numpy(scene).cuda(), n, overlap=overlap, batch=batch), got)
    random.seed(5)                                 # integer sums: another batch grouping adds the same words
    assert np.array_equal(super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=6), got)


# ---------------------------------------------------------------- 4. the driver's `overlap:` option
def _driver_setup(tmp_path, weights):
    from PIL import Image
    from oracle import make_infer_golden as M
    os.makedirs(tmp_path / "scenes", exist_ok=True)
    rng = np.random.RandomState(8)
    yy, xx = np.mgrid[0:40, 0:72]
    base = 110 + 60 * np.sin(yy / 7.0)[None, :, :, None] * np.cos(xx / 11.0)[None, :, :, None]
    a = np.clip(base + rng.randint(-20, 21, size=(3, 40, 72, 3)), 1, 255).astype(np.uint8)
    b = np.clip(base[::-1] + rng.randint(-20, 21, size=(2, 40, 72, 3)), 1, 255).astype(np.uint8)
    np.save(tmp_path / "scenes" / "a.npy", a)
    Image.fromarray(b.reshape(80, 72, 3)).save(tmp_path / "scenes" / "b.png")
    opt = yaml.safe_load(M.option_text(str(tmp_path / "scenes") + "/", str(tmp_path / "out") + "/", weights))
    opt["scene_hw"] = [40, 72]
    opt["io_workers"] = 2
    return opt, a, b


def test_driver_with_overlap_takes_scenes_of_any_size(tmp_path):
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.infer_grid import load_generator
    from satlas_super_resolution_amd.infer_scene import run_infer_scene, super_resolve_scene_blended
    M.write_weights(str(tmp_path / "w.pth"))
    opt, a, b = _driver_setup(tmp_path, str(tmp_path / "w.pth"))
    with pytest.raises(ValueError, match="40 x 72"):                     # without the option: the present path and its refusal
        run_infer_scene(dict(opt))
    assert not os.path.exists(tmp_path / "out") or not _pngs(str(tmp_path / "out"))
    random.seed(3)
    res = run_infer_scene(dict(opt, overlap=8))
    assert (res["scenes"], res["chunks"]) == (2, 2 * 2 * 3) and res["seconds"] > 0
    assert _pngs(str(tmp_path / "out")) == ["a/stitched_s2.png", "a/stitched_sr.png", "b/stitched_s2.png", "b/stitched_sr.png"]
    assert np.array_equal(_png(tmp_path / "out" / "a" / "stitched_s2.png"), a[0])
    assert np.array_equal(_png(tmp_path / "out" / "b" / "stitched_s2.png"), b[0])
    model = load_generator(opt, torch.device("cuda"))
    random.seed(3)                                 # the driver's draws: scene a's chunks, then scene b's
    for name, s in (("a", a), ("b", b)):
        sr = _png(tmp_path / "out" / name / "stitched_sr.png")
        assert sr.shape == (160, 288, 3) and float(sr.std()) > 5
        assert np.array_equal(sr, super_resolve_scene_blended(model, s, 1, overlap=8)), name
    with pytest.raises(ValueError, match="overlap"):
        run_infer_scene(dict(opt, overlap=17, save_path=str(tmp_path / "out17") + "/"))


def test_driver_with_overlap_refuses_non_finite_outputs(tmp_path):
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.infer_scene import run_infer_scene
    sd = dict(M.write_weights(str(tmp_path / "good.pth")))
    w = sd["conv_first.weight"].clone()
    w.view(-1)[0] = 100.0                  # beyond fp32h's packed-weight range (|w| < 64)
    sd["conv_first.weight"] = w
    bad = str(tmp_path / "bad.pth")
    torch.save({"params_ema": sd, "params": sd}, bad)
    opt, _, _ = _driver_setup(tmp_path, bad)
    os.remove(tmp_path / "scenes" / "b.png")
    opt.update(overlap=8, compute_dtype="fp32h")
    with pytest.raises(FloatingPointError, match="fp32f") as e:
        run_infer_scene(opt)
    assert "scene a" in str(e.value)                                          # names the scene
    assert not os.path.exists(tmp_path / "out") or not _pngs(str(tmp_path / "out"))
