"""GPU: the `frame_select: clearest` policy of scene inference (satlas_super_resolution_amd/infer_scene.py; ssr_scene_frame_keys and
ssr_scene_rank_frames of csrc/scene.hip) - the two kernels against the numpy restatement of tests/test_scene_select_host.py
(`window_counts`, `lexsort_rank`), `super_resolve_scene(_blended)(..., frame_select="clearest")` on the grid, blended and bands paths
against mosaics assembled here from the public pieces with frame ids from that restatement, and the driver's option.  Every
comparison is exact.  Fixture-sized generators only (num_feat 16, num_block 1)."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from test_gpu_scene_bands import _odd_base, _png, _pngs, _small_model
from test_scene_blend_host import blend_reference, grid_of
from test_scene_select_host import keys_of, lexsort_rank, window_counts

pytestmark = pytest.mark.gpu


def _u32(t):
    """an int32-storage device tensor as the uint32 words it holds (int64 on the host)"""
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


# ---------------------------------------------------------------- 1. the keys kernel
def test_frame_keys_equal_the_numpy_counts_at_any_origin_and_alignment():
    """3 W = 135 bytes per scene row: the rows of a window start at every byte offset of a word, whatever the base pointer.  Zeros
    and 255s are planted per byte (about 5 % each) and whole (255, 255, 255) pixels on top, so both halves of the key are busy."""
    from satlas_super_resolution_amd.infer_scene import scene_frame_keys
    rng = np.random.RandomState(7)
    T, H, W = 5, 70, 45
    scene = rng.randint(1, 255, size=(T, H, W, 3)).astype(np.uint8)
    u = rng.rand(T, H, W, 3)
    scene[u < 0.05] = 0
    scene[u > 0.95] = 255
    scene[rng.rand(T, H, W) < 0.05] = 255
    scene[0, 3, 4] = (255, 255, 254)               # not saturated, no zero: in neither count
    scene[0, 3, 5] = (0, 255, 255)                 # a zero: in z only
    scene[1, 40, 13] = (0, 9, 9)                   # the first byte of row 2 of the window at (38, 13)
    scene[1, 40, 44] = (255, 255, 255)             # the last pixel of that row
    scene[1, 39, 12] = (9, 9, 0)                   # the pixel before the first of row 1 of the window at (38, 13): not its own
    scene[3] = 0                                   # z = 1024
    scene[4] = 255                                 # s = 1024
    origins = [(0, 0), (38, 13), (37, 12), (H - 32, W - 32), (39, 0), (0, 14), (-1, 0)]          # the last three: outside the scene
    inside = 4
    z, s = window_counts(scene, origins[:inside])
    assert (z[:, 3] == 1024).all() and (s[:, 3] == 0).all() and (s[:, 4] == 1024).all() and (z[:, 4] == 0).all()
    assert (z + s <= 1024).all() and z[:, :3].min() > 50 and s[:, :3].min() > 20
    want = keys_of(z, s)
    org = torch.tensor(origins, dtype=torch.int32, device="cuda")
    for name, dev in (("aligned", torch.from_numpy(scene).cuda()), ("odd base", _odd_base(scene))):
        out = torch.full((len(origins), T), -7, dtype=torch.int32, device="cuda")
        got = scene_frame_keys(dev, org, out)
        torch.cuda.synchronize()
        assert got is out
        got = _u32(got)
        print(f"[{name}] differing keys {int((got[:inside] != want).sum())} of {want.size}")
        assert np.array_equal(got[:inside], want), name
        assert (out[inside:].cpu().numpy() == -7).all(), name            # rows of origins outside the scene are not written
    fresh = scene_frame_keys(torch.from_numpy(scene).cuda(), org)        # without `out`: zeros where nothing is written
    assert np.array_equal(_u32(fresh)[:inside], want) and not fresh[inside:].any()


# ---------------------------------------------------------------- 2. the rank kernel
@pytest.mark.parametrize("T", [1, 2, 5, 64, 65, 130])
def test_rank_frames_equals_lexsort(T):
    """64 frames fill the wave once, 65 and 130 go round the strided loop; keys above 2^31 check the unsigned comparison"""
    from satlas_super_resolution_amd.infer_scene import scene_rank_frames
    rng = np.random.RandomState(T)
    chunks = 7
    few = rng.choice(np.array([0, 3, 1 << 16, (1024 << 16)], np.int64), size=(chunks, T))        # ties everywhere
    wide = rng.randint(0, 1 << 32, size=(chunks, T), dtype=np.int64)
    wide[0, 0] = 0xFFFFFFFF
    for name, key in (("4 values", few), ("random", wide)):
        dev = torch.from_numpy(key.astype(np.uint32).view(np.int32)).cuda()
        for n in sorted({1, min(8, T), T}):
            got = scene_rank_frames(dev, n)
            torch.cuda.synchronize()
            assert got.dtype == torch.int32 and tuple(got.shape) == (chunks, n)
            got = got.cpu().numpy()
            assert np.array_equal(got, lexsort_rank(key, n)), (name, T, n)
            for row in got.tolist():                                     # a prefix of a permutation: no id twice, none outside
                assert len(set(row)) == n and min(row) >= 0 and max(row) < T


# ---------------------------------------------------------------- 3. end to end
@functools.lru_cache(maxsize=None)
def _model(c_in):
    return _small_model(c_in)


def _scene(seed, T, H, W):
    """frame 0 clean but 80 % saturated, the others clean and unsaturated but for what is planted: what `clearest` takes varies from
    chunk to chunk and is never frame 0, which `random` draws as readily as any other clean frame"""
    assert T == 5
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    tci = np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 254).astype(np.uint8)
    tci[0][rng.rand(H, W) < 0.8] = 255
    tci[1, :, 40] = 0                              # frame 1 holds zeros wherever a window covers column 40
    tci[2, 20:22, 5:7] = 255                       # frame 2: 4 saturated pixels near the top left
    tci[2, 40:42, 70:72] = 255                     # and 4 in the lower right of the wide scenes (outside the narrow one)
    tci[3, 10:14, 10:14] = 255                     # frame 3: 16 of them
    tci[4, H - 3, W - 3] = (255, 255, 255)         # frame 4: one in the last window
    tci[4, 5, 20, 1] = 0                           # and one NODATA pixel in the first
    return tci


def _clearest_ids(tci, origins, n):
    z, s = window_counts(tci, origins)
    return lexsort_rank(keys_of(z, s), n)


def _random_ids(tci, origins, n, seed):
    from satlas_super_resolution_amd.infer_scene import select_scene_frames
    z, _ = window_counts(tci, origins)
    random.seed(seed)
    return select_scene_frames(z > 0, n)


def _run_chunks(model, gather, origins):
    """gather -> run_forward for all the chunks as one batch: (the plan, whose `out` holds the chunks' outputs)"""
    plan = model.plan_for_inference(len(origins), 32, 32)
    with torch.no_grad():
        gather(plan)
        model.run_forward(plan)
    return plan


def _scattered(plan, n_chunks, H, W):
    from satlas_super_resolution_amd.infer_scene import scene_scatter_u8
    mosaic = torch.zeros(4 * H, 4 * W, 3, dtype=torch.uint8, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    scene_scatter_u8(plan.out, torch.arange(n_chunks, dtype=torch.int32, device="cuda"), 3, mosaic, counter, plan.dt)
    torch.cuda.synchronize()
    assert int(counter[0]) == 0
    return mosaic.cpu().numpy()


def _policy_checks(call, want, tci, origins, n, monkeypatch):
    """what every path is held to: `clearest` is the assembled mosaic whatever the `random` module holds and without consuming it,
    `random` is today's call, and the two differ"""
    from satlas_super_resolution_amd import infer_scene
    random.seed(1)
    state = random.getstate()
    got = call(frame_select="clearest").copy()
    assert random.getstate() == state                                    # nothing was drawn
    print(f"differing bytes {int((got != want).sum())} of {want.size}")
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert float(got.std()) > 5
    random.seed(2)
    with monkeypatch.context() as m:                                     # and neither the flags nor the host's choice are asked for
        for name in ("scene_zero_scan", "scene_zero_scan_at", "select_scene_frames"):
            m.setattr(infer_scene, name, None)
        assert np.array_equal(call(frame_select="clearest"), got)
    assert not np.array_equal(_random_ids(tci, origins, n, 5), _clearest_ids(tci, origins, n))
    random.seed(5)
    today = call().copy()
    random.seed(5)
    assert np.array_equal(call(frame_select="random"), today)
    assert random.getstate() != state
    assert not np.array_equal(today, got)                                # a `clearest` that fell back to `random` cannot pass


def test_grid_path_with_clearest_frames_is_the_public_pieces_on_the_restated_choice(monkeypatch):
    from satlas_super_resolution_amd.infer_scene import scene_gather, super_resolve_scene
    T, H, W, n = 5, 64, 96, 2
    tci = _scene(31, T, H, W)
    origins = grid_of(H, W, 0)
    ids = _clearest_ids(tci, origins, n)
    assert len({tuple(r) for r in ids.tolist()}) >= 3 and not (ids == 0).any()       # the choice varies, frame 0 is never taken
    model = _model(3 * n)
    dev = torch.from_numpy(tci).cuda()
    plan = _run_chunks(model, lambda p: scene_gather(dev, torch.arange(len(origins), dtype=torch.int32, device="cuda"),
                                                     torch.from_numpy(ids).cuda(), p.xin, p.dt), origins)
    want = _scattered(plan, len(origins), H, W)
    _policy_checks(lambda **kw: super_resolve_scene(model, tci, n, batch=4, **kw), want, tci, origins, n, monkeypatch)
    assert np.array_equal(super_resolve_scene(model, dev, n, frame_select="clearest"), want)         # a device tensor, one batch


def test_blended_path_with_clearest_frames_is_the_public_pieces_on_the_restated_choice(monkeypatch):
    from satlas_super_resolution_amd.infer_scene import scene_gather_at, super_resolve_scene_blended
    T, H, W, n, overlap = 5, 70, 45, 2, 8
    tci = _scene(32, T, H, W)
    origins = grid_of(H, W, overlap)
    assert origins == [(0, 0), (0, 13), (24, 0), (24, 13), (38, 0), (38, 13)]
    ids = _clearest_ids(tci, origins, n)
    assert len({tuple(r) for r in ids.tolist()}) >= 2 and not (ids == 0).any()
    model = _model(3 * n)
    dev = torch.from_numpy(tci).cuda()
    plan = _run_chunks(model, lambda p: scene_gather_at(dev, torch.tensor(origins, dtype=torch.int32, device="cuda"),
                                                        torch.from_numpy(ids).cuda(), p.xin, p.dt), origins)
    torch.cuda.synchronize()
    want = blend_reference(plan.out[..., :3].float().cpu().numpy(), origins, H, W, overlap)
    _policy_checks(lambda **kw: super_resolve_scene_blended(model, tci, n, overlap=overlap, batch=4, **kw), want, tci, origins, n,
                   monkeypatch)


def test_bands_path_with_clearest_frames_is_the_public_pieces_on_the_restated_choice(monkeypatch):
    from satlas_super_resolution_amd.infer_scene import scene_gather_bands, super_resolve_scene
    T, H, W, n, K = 5, 64, 96, 2, 1
    tci = _scene(33, T, H, W)
    rng = np.random.RandomState(34)
    bands = rng.randint(0, 256, size=(K, T, H, W)).astype(np.uint8)      # zeros and 255s in a band: no part in the choice
    bands[0, 3:] = 0
    origins = grid_of(H, W, 0)
    ids = _clearest_ids(tci, origins, n)
    model = _model(n * (3 + K))
    dev, bdev = torch.from_numpy(tci).cuda(), torch.from_numpy(bands).cuda()
    plan = _run_chunks(model, lambda p: scene_gather_bands(dev, bdev, torch.tensor(origins, dtype=torch.int32, device="cuda"),
                                                           torch.from_numpy(ids).cuda(), p.xin, p.dt), origins)
    want = _scattered(plan, len(origins), H, W)
    _policy_checks(lambda **kw: super_resolve_scene(model, tci, n, batch=4, bands=bands, **kw), want, tci, origins, n, monkeypatch)


# ---------------------------------------------------------------- 4. the driver's `frame_select:` option
def test_driver_with_frame_select_clearest(tmp_path):
    from PIL import Image
    from satlas_super_resolution_amd.infer_scene import run_infer_scene, super_resolve_scene
    T, H, W, n = 5, 64, 96, 2
    scenes = {"a": _scene(41, T, H, W), "b": _scene(42, T, H, W)}
    os.makedirs(tmp_path / "scenes")
    Image.fromarray(scenes["a"].reshape(T * H, W, 3)).save(tmp_path / "scenes" / "a.png")
    np.save(tmp_path / "scenes" / "b.npy", scenes["b"])
    model = _model(3 * n)
    opt = {"data_dir": str(tmp_path / "scenes") + "/", "save_path": str(tmp_path / "out") + "/", "n_lr_images": n, "scene_hw": [H, W],
           "io_workers": 2, "frame_select": "clearest"}
    random.seed(9)
    state = random.getstate()
    res = run_infer_scene(opt, model=model)
    assert random.getstate() == state
    assert res["frame_select"] == "clearest" and (res["scenes"], res["chunks"]) == (2, 12)
    assert _pngs(str(tmp_path / "out")) == [f"{k}/stitched_{m}.png" for k in "ab" for m in ("s2", "sr")]
    for name, tci in scenes.items():
        want = super_resolve_scene(model, tci, n, frame_select="clearest")
        assert np.array_equal(_png(tmp_path / "out" / name / "stitched_sr.png"), want), name
        assert np.array_equal(_png(tmp_path / "out" / name / "stitched_s2.png"), tci[0]), name         # frame 0 under both policies
        random.seed(9)
        assert not np.array_equal(super_resolve_scene(model, tci, n), want), name
    res = run_infer_scene(dict(opt, frame_select="random", save_path=str(tmp_path / "out2") + "/"), model=model)
    assert res["frame_select"] == "random" and random.getstate() != state
