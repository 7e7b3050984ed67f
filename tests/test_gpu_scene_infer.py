"""GPU: scene inference (satlas_super_resolution_amd/infer_scene.py, csrc/scene.hip) - the three kernels against numpy and the
existing converters (exact), the driver against what the UNMODIFIED reference infer_grid.py wrote for the same pixels
(tests/golden/infer_scripts.pt, the gate tests/test_gpu_infer_scripts.py applies to the chunked driver), byte identity with the
chunked path, the non-finite refusal and the command line under two ranks.  Fixture-sized generators only (num_feat 16, num_block 1)."""
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk_stacks(scene):
    """uint8 [T, H, W, 3] -> [gh*gw, T, 32, 32, 3], chunks in row-major order"""
    T, H, W, _ = scene.shape
    return scene.reshape(T, H // 32, 32, W // 32, 32, 3).transpose(1, 3, 0, 2, 4, 5).reshape(-1, T, 32, 32, 3)


def _paste(mosaic, cell, chunk_id):
    gw = mosaic.shape[1] // cell.shape[1]
    i, j = divmod(int(chunk_id), gw)
    s = cell.shape[0]
    mosaic[s * i:s * (i + 1), s * j:s * (j + 1)] = cell


def _levels(a, b):
    d = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return int(d.max()), float((d > 0).mean())


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB")).copy()


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


# ---------------------------------------------------------------- 1. kernels against numpy, exact
def test_zero_scan_finds_planted_zeros_and_nothing_else():
    from satlas_super_resolution_amd.infer_scene import scene_zero_scan
    rng = np.random.RandomState(11)
    T, H, W = 5, 64, 96
    scene = rng.randint(1, 256, size=(T, H, W, 3)).astype(np.uint8)
    gw = W // 32
    # (chunk, frame, byte of the 3072 of that frame of that chunk): first and last byte, a row end, a row start, the middle
    planted = [(0, 0, 0), (0, 3, 3071), (2, 1, 95), (3, 4, 96), (5, 2, 1537), (5, 4, 3071), (4, 0, 3070), (1, 2, 1)]
    for chunk, t, byte in planted:
        i, j = divmod(chunk, gw)
        row, col = divmod(byte, 96)
        scene[t, 32 * i + row, 32 * j + col // 3, col % 3] = 0
    want = (_chunk_stacks(scene) == 0).any(axis=(2, 3, 4))
    assert int(want.sum()) == len(planted)
    got = scene_zero_scan(torch.from_numpy(scene).cuda()).cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == (6, T)
    assert np.array_equal(got, want.astype(np.uint8))
    clean = scene_zero_scan(torch.from_numpy(np.maximum(scene, 1)).cuda()).cpu().numpy()
    assert not clean.any()


@pytest.mark.parametrize("storage,n,cs", [("fp32", 3, 16), ("fp32", 4, 16), ("fp32", 8, 24), ("fp32", 5, 16),
                                          ("bf16", 3, 16), ("bf16", 8, 32), ("bf16", 8, 24)])
def test_gather_equals_frames_to_input_and_the_layout_converter(storage, n, cs):
    """9 / 15 channels: element stores; 12 (fp32) and 24 channels: 16-byte stores; every view but the 24-wide one has a channel pad,
    which must keep what it held"""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import scene_gather
    from satlas_super_resolution_amd.utils.infer_utils import frames_to_input
    rng = np.random.RandomState(5)
    T, H, W = 8, 64, 96
    scene = rng.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    assert len(np.unique(scene)) == 256                                  # every byte value goes through the division
    chunk_ids = np.array([4, 0, 5, 2, 2, 1, 3], np.int32)               # shuffled, one chunk twice
    B = len(chunk_ids)
    frame_ids = np.stack([rng.permutation(T)[:n] for _ in range(B)]).astype(np.int32)
    stacks = _chunk_stacks(scene)
    sel = np.stack([stacks[c][f] for c, f in zip(chunk_ids, frame_ids)])                 # [B, n, 32, 32, 3]
    dt = hip.dtype_code(storage)
    tdt = hip.torch_dtype(dt)
    x = frames_to_input(torch.from_numpy(sel).cuda()).contiguous()
    want = torch.full((B, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    hip.check(hip.lib().ssr_nchw_to_nhwc(x.data_ptr(), B, 3 * n, 32, 32, hip.view(want), dt, 1, 1, 1.0, hip.stream_ptr()), "ssr_nchw_to_nhwc")
    got = torch.full((B, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    scene_gather(torch.from_numpy(scene).cuda(), torch.from_numpy(chunk_ids).cuda(), torch.from_numpy(frame_ids).cuda(), got, dt)
    torch.cuda.synchronize()
    diff = (got.float() - want.float()).abs()
    print(f"[{storage}, n = {n}, cs = {cs}] differing elements {int((got != want).sum())} of {got.numel()}, largest difference {float(diff.max()):.3e}")
    assert torch.equal(got, want)
    assert bool((got[..., 3 * n:] == -7.0).all()) and float(got[..., :3 * n].float().min()) >= 0.0


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_scatter_equals_the_checked_quantiser_pasted_by_numpy(storage):
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import scene_scatter_u8
    from satlas_super_resolution_amd.metrics import quantize_u8_checked, split_checked
    g = torch.Generator().manual_seed(9)
    B, C, cs = 4, 3, 8
    buf = torch.rand(B, 128, 128, cs, generator=g) * 1.6 - 0.3           # values below 0 and above 1
    k = torch.randint(0, 256, (B, 128, 32, cs), generator=g).float()
    near = k / 255                                                        # within one ulp of k / 255, on both sides
    near = torch.where(torch.rand(near.shape, generator=g) < 0.5, torch.nextafter(near, torch.tensor(2.0)), torch.nextafter(near, torch.tensor(-1.0)))
    buf[:, :, :32] = near
    buf[:, :, 32:40] = k[:, :, :8] / 255
    buf[1, 5, 77, 2] = float("nan")
    buf[3, 127, 127, 0] = float("nan")
    buf[2, 64, 3, 5] = float("nan")                                       # a pad channel: not an output sample
    dt = hip.dtype_code(storage)
    src = buf.to(hip.torch_dtype(dt)).cuda().contiguous()
    x = src[..., :C].float().permute(0, 3, 1, 2).contiguous()             # what ssr_nhwc_to_nchw hands the chunked path
    img, bad = split_checked(*quantize_u8_checked(x, truncate=True))
    img = img.cpu().numpy()
    assert bad == 2
    chunk_ids = np.array([5, 0, 3, 1], np.int32)                          # of a 2 x 3 grid: cells 2 and 4 are not written
    want = np.full((256, 384, C), 7, np.uint8)
    for b, c in enumerate(chunk_ids):
        _paste(want, img[b], c)
    mosaic = torch.full((256, 384, C), 7, dtype=torch.uint8, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    scene_scatter_u8(src, torch.from_numpy(chunk_ids).cuda(), C, mosaic, counter, dt)
    torch.cuda.synchronize()
    assert int(counter[0]) == 2
    got = mosaic.cpu().numpy()
    assert np.array_equal(got, want)
    assert len(np.unique(got)) > 200


# ---------------------------------------------------------------- 2. against the unmodified reference script
def _golden_setup(tmp_path):
    from oracle import make_infer_golden as M
    M.write_weights(str(tmp_path / "w.pth"))
    os.makedirs(tmp_path / "scenes")
    t0 = np.zeros((1, 512, 512, 3), np.uint8)
    for i in range(16):
        for j in range(16):
            t0[0, 32 * i:32 * (i + 1), 32 * j:32 * (j + 1)] = M.chunk_image(0, i, j)
    from PIL import Image
    Image.fromarray(t0.reshape(512, 512, 3)).save(tmp_path / "scenes" / "t0.png")
    t1 = np.concatenate([M.chunk_image(1, 0, j) for j in range(3)], axis=1)[None]          # the reference tree's incomplete tile
    np.save(tmp_path / "scenes" / "t1.npy", t1)
    opt = yaml.safe_load(M.option_text(str(tmp_path / "scenes") + "/", str(tmp_path / "out") + "/", str(tmp_path / "w.pth")))
    return M, opt


@pytest.mark.parametrize("compute_dtype", ["fp32h", "fp32x3", "fp32"])
def test_scene_driver_matches_the_unmodified_reference_script(tmp_path, compute_dtype):
    from satlas_super_resolution_amd.infer_scene import run_infer_scene
    fx = load_golden("infer_scripts")
    M, opt = _golden_setup(tmp_path)
    opt["compute_dtype"] = compute_dtype
    res = run_infer_scene(opt)
    assert (res["scenes"], res["chunks"]) == (2, 259) and res["seconds"] > 0
    assert _pngs(str(tmp_path / "out")) == ["t0/stitched_s2.png", "t0/stitched_sr.png", "t1/stitched_s2.png", "t1/stitched_sr.png"]
    assert M.digest(_png(tmp_path / "out" / "t0" / "stitched_s2.png")) == fx["grid_stitched_s2_sha256"]      # input mosaic: exact
    sr, sr1 = _png(tmp_path / "out" / "t0" / "stitched_sr.png"), _png(tmp_path / "out" / "t1" / "stitched_sr.png")
    assert sr.shape == (2048, 2048, 3) and sr1.shape == (128, 384, 3)
    worst, frac = 0, 0.0
    for key, ref in fx["grid_chunks"].items():
        tile, cell = key[:-4].split("/")
        i, j = (int(v) for v in cell.split("_"))
        ours = (sr if tile == "t0" else sr1)[128 * i:128 * (i + 1), 128 * j:128 * (j + 1)]
        mx, fr = _levels(ours, ref.numpy())
        worst, frac = max(worst, mx), max(frac, fr)
    mx, fr = _levels(sr[::8, ::8], fx["grid_stitched_sr_sub8"].numpy())
    mx2, _ = _levels(sr[640], fx["grid_stitched_sr_row640"].numpy())
    print(f"[{compute_dtype}] scene driver against the reference script: worst difference {max(worst, mx, mx2)} level(s), "
          f"fraction of differing samples <= {max(frac, fr):.2e}")
    assert max(worst, mx, mx2) <= 1 and max(frac, fr) <= 2e-3
    assert float(sr.std()) > 5                                           # real images, not a constant


# ---------------------------------------------------------------- 3. byte identity with the chunked path
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


def test_scene_result_is_the_chunked_paths_bytes():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene
    from satlas_super_resolution_amd.utils.infer_utils import frames_to_input, quantize_output, select_frames
    rng = np.random.RandomState(21)
    T, H, W, n, batch = 4, 64, 96, 2, 4
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    scene = np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 255).astype(np.uint8)
    scene[0, 3, 5, 1] = 0                          # chunk 0: one zero-holding frame
    scene[1, 40, 70, 0] = scene[2, 41, 71, 2] = scene[3, 63, 95, 2] = 0          # chunk 5: one clean frame, topped up
    scene[:, 33, 1, 0] = 0                         # chunk 3: every frame holds a zero
    model = _small_model(n)
    random.seed(5)
    got = super_resolve_scene(model, scene, n, batch=batch)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    got = got.copy()
    # the chunked path: select_frames chunk by chunk in row-major order, the same batch grouping (a full batch and a ragged one)
    stacks = _chunk_stacks(scene)
    random.seed(5)
    sels = [select_frames(s.reshape(T * 32, 32, 3), n)[0] for s in stacks]
    want = np.zeros_like(got)
    with torch.no_grad():
        for c0 in range(0, len(sels), batch):
            x = frames_to_input(torch.from_numpy(np.stack(sels[c0:c0 + batch])).cuda())
            y = quantize_output(model(x), model.compute_dtype)
            for k in range(y.shape[0]):
                _paste(want, y[k], c0 + k)
    assert np.array_equal(got, want)
    assert float(got.std()) > 5
    random.seed(5)
    assert np.array_equal(super_resolve_scene(model, scene, n, batch=batch), got)                       # replayed graphs: same bytes
    random.seed(5)
    assert np.array_equal(super_resolve_scene(model, torch.from_numpy(scene).cuda(), n, batch=batch), got)      # a device tensor
    with pytest.raises(ValueError):                # five frames of four: random.sample, as in the reference
        super_resolve_scene(_small_model(5), scene, 5, batch=batch)


# ---------------------------------------------------------------- 4. non-finite outputs
def test_scene_driver_refuses_non_finite_outputs(tmp_path):
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.infer_scene import run_infer_scene
    sd = dict(M.write_weights(str(tmp_path / "good.pth")))
    w = sd["conv_first.weight"].clone()
    w.view(-1)[0] = 100.0                  # beyond fp32h's packed-weight range (|w| < 64)
    sd["conv_first.weight"] = w
    bad = str(tmp_path / "bad.pth")
    torch.save({"params_ema": sd, "params": sd}, bad)
    os.makedirs(tmp_path / "scenes")
    np.save(tmp_path / "scenes" / "t1.npy", np.concatenate([M.chunk_image(1, 0, j) for j in range(3)], axis=1)[None])

    def opt(out, dtype):
        o = yaml.safe_load(M.option_text(str(tmp_path / "scenes") + "/", str(tmp_path / out) + "/", bad))
        o["compute_dtype"] = dtype
        return o

    with pytest.raises(FloatingPointError, match="fp32f") as e:
        run_infer_scene(opt("o_h", "fp32h"))
    assert "t1" in str(e.value)                                           # names the scene
    assert not os.path.exists(tmp_path / "o_h") or not _pngs(str(tmp_path / "o_h"))
    res = run_infer_scene(opt("o_f", "fp32f"))                            # the same checkpoint in exact fp32
    assert (res["scenes"], res["chunks"]) == (1, 3)
    assert _pngs(str(tmp_path / "o_f")) == ["t1/stitched_s2.png", "t1/stitched_sr.png"]


# ---------------------------------------------------------------- 5. the command line under two ranks
def test_two_ranks_write_their_own_scenes(tmp_path):
    """`python -m torch.distributed.run --nproc-per-node 2 -m satlas_super_resolution_amd.infer_scene -opt ...` as two processes on
    this GPU (gloo standing in for RCCL, as tests/test_gpu_infer_scripts.py launches infer_grid).  Every chunk has exactly one frame
    without a zero, so the frame choice does not depend on the ranks' unseeded `random` streams."""
    from PIL import Image
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.infer_grid import load_generator
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene
    M.write_weights(str(tmp_path / "w.pth"))
    os.makedirs(tmp_path / "scenes")
    rng = np.random.RandomState(2)
    scenes = {}
    for name in ("a", "b", "c"):
        s = rng.randint(1, 256, size=(2, 64, 64, 3)).astype(np.uint8)
        for k in range(4):                          # chunk k: frame k % 2 holds a zero, the other one is the choice
            i, j = divmod(k, 2)
            s[k % 2, 32 * i + 7, 32 * j + 9, 1] = 0
        scenes[name] = s
        if name == "b":
            np.save(tmp_path / "scenes" / "b.npy", s)
        else:
            Image.fromarray(s.reshape(128, 64, 3)).save(tmp_path / "scenes" / f"{name}.png")
    opt = yaml.safe_load(M.option_text(str(tmp_path / "scenes") + "/", str(tmp_path / "out") + "/", str(tmp_path / "w.pth")))
    opt["io_workers"] = 2
    with open(tmp_path / "opt.yml", "w") as f:
        yaml.safe_dump(opt, f)
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0",
                   SSR_DIST_BACKEND="gloo", PYTHONPATH=ROOT)
        procs.append(subprocess.Popen([sys.executable, "-m", "satlas_super_resolution_amd.infer_scene", "-opt", str(tmp_path / "opt.yml")],
                                      cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert "'scenes': 2" in outs[0] and "'chunks': 8" in outs[0], outs[0]            # rank 0: a and c
    assert "'scenes': 1" in outs[1] and "'chunks': 4" in outs[1], outs[1]            # rank 1: b
    assert _pngs(str(tmp_path / "out")) == [f"{n}/stitched_{k}.png" for n in "abc" for k in ("s2", "sr")]
    model = load_generator(opt, torch.device("cuda"))
    for name, s in scenes.items():
        assert np.array_equal(_png(tmp_path / "out" / name / "stitched_s2.png"), s[0]), name
        want = super_resolve_scene(model, s, 1)
        assert np.array_equal(_png(tmp_path / "out" / name / "stitched_sr.png"), want), name
        assert float(want.std()) > 5


# ---------------------------------------------------------------- 6.
def test_abi_version_is_unchanged():
    from satlas_super_resolution_amd import hip
    assert hip.lib().ssr_abi_version() == 3
