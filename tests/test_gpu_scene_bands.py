"""GPU: multi-band scene inference (satlas_super_resolution_amd/infer_scene.py `bands=` / `s2_bands`, ssr_scene_gather_bands of
csrc/scene.hip) - the gather against numpy and against the dataset's own stacking, `super_resolve_scene` and
`super_resolve_scene_blended` with bands against the module's forward on host-assembled inputs, and the driver on the dataset
fixture's `sentinel2` folder.  Every comparison is exact.  Fixture-sized generators only (num_feat 16, num_block 1)."""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_scene_blend_host import blend_reference, grid_of

pytestmark = pytest.mark.gpu

S2 = os.path.join(GOLDEN, "s2naip_mini", "sentinel2")
INV255 = np.float32(1.0 / 255.0)


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path)).copy()


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def _inside(y0, x0, H, W):
    return 0 <= y0 <= H - 32 and 0 <= x0 <= W - 32


def _rup(c, m):
    return -(-c // m) * m


def _bf16(a):
    """fp32 -> the nearest bf16 (ties to even), widened back to fp32; finite inputs only"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)
    return r.astype(np.uint32).view(np.float32)


def _stack(tci, bands, y0, x0, frames):
    """uint8 [n (3 + K), 32, 32]: per chosen frame the TCI window (channels first), then the K band windows - frame-major"""
    parts = []
    for f in frames:
        parts.append(tci[f, y0:y0 + 32, x0:x0 + 32].transpose(2, 0, 1))
        parts.append(bands[:, f, y0:y0 + 32, x0:x0 + 32])
    return np.concatenate(parts, axis=0)


def _odd_base(a):
    """the array on the device at an odd byte address (a view one byte into a larger buffer)"""
    big = torch.zeros(a.size + 1, dtype=torch.uint8, device="cuda")
    big[1:] = torch.from_numpy(a).cuda().reshape(-1)
    v = big[1:].view(a.shape)
    assert v.data_ptr() % 2 == 1
    return v


# ---------------------------------------------------------------- 1. the gather against numpy
@pytest.mark.parametrize("H,W", [(32, 32), (64, 96), (37, 45)])
@pytest.mark.parametrize("K,n,T", [(1, 1, 1), (2, 1, 2), (1, 2, 3), (9, 2, 3)])       # 4, 5, 8, 24 channels
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_gather_bands_equals_numpy(storage, K, n, T, H, W):
    """4 and 5 channels: element stores in both storages; 8: 16-byte stores; 24: 16-byte stores whose packs straddle the frames'
    12 channels in bf16.  Origins: the first chunk, the corner (H - 32, W - 32), odd x0 wherever the scene is wider than a chunk
    (and the arrays themselves start on odd addresses, W and 3 W are odd for W = 45); one item outside the scene and one with a
    frame id equal to T, which must leave their pixels alone, as every item leaves the pad channels."""
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import scene_gather_bands
    rng = np.random.RandomState(100 * K + 10 * n + T + H)
    tci = rng.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)
    bands = rng.randint(0, 256, size=(K, T, H, W)).astype(np.uint8)
    origins = [(0, 0), (H - 32, W - 32)]
    if W > 32:
        origins += [(3, 1), (H - 32, 13), (0, W - 33)]                   # (W - 32 >= 13 in both wider scenes)
    origins += [(H - 31, 0), (0, 0)]                                     # outside the scene; the item with the bad frame id
    B = len(origins)
    assert W == 32 or any(x0 % 2 for _, x0 in origins[:-2])
    frame_ids = np.stack([np.sort(rng.permutation(T)[:n])[::-1] for _ in range(B)]).astype(np.int32)     # descending
    frame_ids[B - 1, n - 1] = T
    ok = [_inside(y0, x0, H, W) for y0, x0 in origins]
    ok[B - 1] = False
    assert ok[:B - 2] == [True] * (B - 2) and not ok[B - 2]
    C, cs = n * (3 + K), _rup(n * (3 + K), 8)
    want = np.full((B, 32, 32, cs), -7.0, np.float32)
    for b, (y0, x0) in enumerate(origins):
        if ok[b]:
            v = _stack(tci, bands, y0, x0, frame_ids[b]).astype(np.float32) * INV255
            assert v.dtype == np.float32
            want[b, :, :, :C] = (_bf16(v) if storage == "bf16" else v).transpose(1, 2, 0)
    dt = hip.dtype_code(storage)
    got = torch.full((B, 32, 32, cs), -7.0, dtype=hip.torch_dtype(dt), device="cuda")
    scene_gather_bands(_odd_base(tci), _odd_base(bands), torch.tensor(origins, dtype=torch.int32, device="cuda"),
                       torch.from_numpy(frame_ids).cuda(), got, dt)
    torch.cuda.synchronize()
    got = got.float().cpu().numpy()
    print(f"[{storage} K = {K} n = {n} T = {T} {H} x {W}] differing elements {int((got != want).sum())} of {got.size}")
    assert np.array_equal(got, want)
    assert (got[..., C:] == -7.0).all() and (got[B - 2:] == -7.0).all() and got[0, ..., :C].min() >= 0.0


def test_gather_bands_stacks_what_the_dataset_stacks():
    from satlas_super_resolution_amd.data.s2naip_dataset import S2NAIPDataset
    from satlas_super_resolution_amd.infer_scene import scene_gather_bands
    mini = os.path.join(GOLDEN, "s2naip_mini")
    ds = S2NAIPDataset({"phase": "val", "scale": 4, "name": "mini", "type": "S2NAIPDataset", "n_s2_images": 2, "s2_bands": ["b08", "tci"],
                        "sentinel2_path": S2, "naip_path": os.path.join(mini, "naip")})
    assert ds.s2_bands == ["tci", "b08"]
    paths = [os.path.join(S2, "100_200", b + ".png") for b in ds.s2_bands]
    lr = ds._load_s2(paths)
    assert tuple(lr.shape) == (10, 4, 32, 32) and lr.dtype == torch.uint8
    want = (lr[[3, 0]].reshape(-1, 32, 32).numpy().astype(np.float32) * INV255).transpose(1, 2, 0)
    tci = _png(paths[0]).reshape(10, 32, 32, 3)
    b08 = _png(paths[1]).reshape(1, 10, 32, 32)
    got = torch.full((1, 32, 32, 8), -7.0, device="cuda")
    scene_gather_bands(torch.from_numpy(tci).cuda(), torch.from_numpy(b08).cuda(), torch.zeros(1, 2, dtype=torch.int32, device="cuda"),
                       torch.tensor([[3, 0]], dtype=torch.int32, device="cuda"), got)
    torch.cuda.synchronize()
    assert np.array_equal(got[0].cpu().numpy(), want)
    assert len(np.unique(want)) > 100


# ---------------------------------------------------------------- 2. end to end
def _small_model(c_in, compute_dtype="fp32h"):
    from oracle import esrgan_oracle as O
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    assert M.G_KW == dict(num_feat=16, num_block=1, num_grow_ch=8)
    sd = O.generator_init(num_in_ch=c_in, num_out_ch=3, scale=4, seed=M.SEED, **M.G_KW)
    sd["conv_last.bias"] = torch.full_like(sd["conv_last.bias"], 0.45)
    sd["conv_last.weight"] = sd["conv_last.weight"] * 8
    net = SSR_RRDBNet(num_in_ch=c_in, num_out_ch=3, compute_dtype=compute_dtype, **M.G_KW)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval().freeze_packed()


def _scene(seed, T, H, W, K):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    tci = np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 255).astype(np.uint8)
    bands = np.clip(base[..., 0][None] * 0.8 + rng.randint(-40, 41, size=(K, T, H, W)), 0, 255).astype(np.uint8)
    bands[0, :, 7, 9] = 0                          # zeros in a band do not make a frame a dirty one
    return tci, bands


def _chosen(tci, origins, n):
    """`select_scene_frames` on flags computed on the host, in the order of the origins"""
    from satlas_super_resolution_amd.infer_scene import select_scene_frames
    flags = np.stack([(tci[:, y0:y0 + 32, x0:x0 + 32] == 0).any(axis=(1, 2, 3)) for y0, x0 in origins])
    return flags, select_scene_frames(flags, n)


def _forward(model, tci, bands, origins, frame_ids, batch):
    """the module's own forward on the host-assembled inputs, `batch` chunks at a time -> fp32 [chunks, 3, 128, 128] (device)"""
    outs = []
    with torch.no_grad():
        for c0 in range(0, len(origins), batch):
            sel = np.stack([_stack(tci, bands, y0, x0, f) for (y0, x0), f in zip(origins[c0:c0 + batch], frame_ids[c0:c0 + batch])])
            outs.append(model(torch.from_numpy(sel).cuda().float() / 255).float())
    return torch.cat(outs)


def test_scene_with_bands_is_the_modules_forward_on_the_stacked_chunks():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene
    from satlas_super_resolution_amd.utils.infer_utils import quantize_output
    T, H, W, n, K, batch = 4, 64, 96, 2, 2, 4
    tci, bands = _scene(21, T, H, W, K)
    tci[0, 3, 5, 1] = 0                            # chunk 0: one zero-holding frame
    tci[1, 40, 70, 0] = tci[2, 41, 71, 2] = tci[3, 63, 95, 2] = 0            # chunk 5: one clean frame, topped up
    tci[:, 33, 1, 0] = 0                           # chunk 3: every frame holds a zero
    model = _small_model(n * (3 + K))
    random.seed(5)
    got = super_resolve_scene(model, tci, n, batch=batch, bands=bands)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    got = got.copy()
    origins = grid_of(H, W, 0)
    assert origins == [(32 * i, 32 * j) for i in range(2) for j in range(3)]
    random.seed(5)
    flags, frame_ids = _chosen(tci, origins, n)
    assert flags.sum(axis=1).tolist() == [1, 0, 0, 4, 0, 3]              # clean and dirty frames mix
    y = quantize_output(_forward(model, tci, bands, origins, frame_ids, batch), model.compute_dtype)
    for k, (y0, x0) in enumerate(origins):
        cell = got[4 * y0:4 * y0 + 128, 4 * x0:4 * x0 + 128]
        assert np.array_equal(cell, y[k]), (k, int((cell != y[k]).sum()))
    assert float(got.std()) > 5
    for other in (1, 5, 64):                       # every chunk is its own: the batch grouping does not show
        random.seed(5)
        assert np.array_equal(super_resolve_scene(model, tci, n, batch=other, bands=bands), got), other
    random.seed(5)                                 # device tensors
    assert np.array_equal(super_resolve_scene(model, torch.from_numpy(tci).cuda(), n, batch=batch, bands=torch.from_numpy(bands).cuda()), got)
    random.seed(5)                                 # the bands matter
    assert not np.array_equal(super_resolve_scene(model, tci, n, batch=batch, bands=np.zeros_like(bands)), got)
    with pytest.raises(ValueError, match="10"):    # a TCI-only call into the 10-channel generator: today's refusal
        super_resolve_scene(model, tci, n, batch=batch)


def test_blended_scene_with_bands_is_the_modules_chunks_through_the_numpy_restatement():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene_blended
    T, H, W, n, K, batch, overlap = 4, 40, 72, 2, 2, 4, 8
    tci, bands = _scene(22, T, H, W, K)
    origins = grid_of(H, W, overlap)
    assert origins == [(0, 0), (0, 24), (0, 40), (8, 0), (8, 24), (8, 40)]
    tci[0, 3, 5, 1] = 0                            # in the chunk at (0, 0) only: one zero-holding frame
    tci[1, 39, 70, 0] = tci[2, 38, 71, 2] = tci[3, 39, 71, 2] = 0            # chunk (8, 40) only: one clean frame, topped up
    tci[:, 20, 30, 0] = 0                          # chunks (0, 0), (0, 24), (8, 0), (8, 24): every frame holds a zero
    model = _small_model(n * (3 + K))
    random.seed(5)
    got = super_resolve_scene_blended(model, tci, n, overlap=overlap, batch=batch, bands=bands)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    got = got.copy()
    random.seed(5)
    _, frame_ids = _chosen(tci, origins, n)
    outs = _forward(model, tci, bands, origins, frame_ids, batch).permute(0, 2, 3, 1).cpu().numpy()
    want = blend_reference(outs, origins, H, W, overlap)
    print(f"differing bytes {int((got != want).sum())} of {want.size}")
    assert np.array_equal(got, want)
    assert float(got.std()) > 5
    for other in (1, 6):                           # integer sums: another batch grouping adds the same words
        random.seed(5)
        assert np.array_equal(super_resolve_scene_blended(model, tci, n, overlap=overlap, batch=other, bands=bands), got), other


# ---------------------------------------------------------------- 3. the driver's `s2_bands:` option
def test_driver_with_s2_bands_runs_the_datasets_sentinel2_folder(tmp_path):
    from satlas_super_resolution_amd.infer_scene import run_infer_scene, super_resolve_scene
    n = 2
    model = _small_model(n * 4)
    opt = {"data_dir": S2, "save_path": str(tmp_path / "out") + "/", "n_lr_images": n, "s2_bands": ["b08", "tci"], "io_workers": 2}
    random.seed(3)
    res = run_infer_scene(opt, model=model)
    tiles = ["100_200", "100_201", "101_200", "101_201", "102_200"]
    assert (res["scenes"], res["chunks"]) == (5, 5) and res["seconds"] > 0
    assert _pngs(str(tmp_path / "out")) == [f"{t}/stitched_{k}.png" for t in tiles for k in ("s2", "sr")]
    random.seed(3)                                 # the driver's draws: the tiles in sorted order
    for t in tiles:
        tci = _png(os.path.join(S2, t, "tci.png"))
        T = tci.shape[0] // 32
        assert T == (6 if t == "102_200" else 10)
        tci = tci.reshape(T, 32, 32, 3)
        b08 = os.path.join(S2, t, "b08.png")
        assert os.path.exists(b08) == (t != "101_201")
        bands = _png(b08).reshape(1, T, 32, 32) if os.path.exists(b08) else np.zeros((1, T, 32, 32), np.uint8)      # missing: zeros
        want = super_resolve_scene(model, tci, n, bands=bands)
        assert np.array_equal(_png(tmp_path / "out" / t / "stitched_sr.png"), want), t
        assert np.array_equal(_png(tmp_path / "out" / t / "stitched_s2.png"), tci[0]), t
        assert want.shape == (128, 128, 3) and float(want.std()) > 5
    with pytest.raises(ValueError, match="tci"):
        run_infer_scene(dict(opt, s2_bands=["b08"], save_path=str(tmp_path / "out2") + "/"), model=model)
