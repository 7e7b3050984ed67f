"""CPU: the host half of the `nodata: keep` policy of scene inference (satlas_super_resolution_amd/infer_scene.py) - the package's
numpy statements of the policy, `scene_support` and `apply_nodata`, against brute-force loops written here (`brute_support`,
`brute_apply`), the saturation of the support map that comes back, the option's refusals and the declaration of the two device entry
points.  Every comparison is exact integer equality."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_scene_blend_host import grid_of

ENTRIES = ("ssr_scene_support_add", "ssr_scene_apply_nodata")


# ---------------------------------------------------------------- the policy, pixel by pixel
def brute_support(tci, origins, frame_ids):
    """int64 [H, W]: for every chunk inside the scene whose frame ids are all frames of the scene, every slot and every pixel of the
    32 x 32 window, one count if none of the pixel's three samples is 0"""
    T, H, W, _ = tci.shape
    px = tci.tolist()
    sup = [[0] * W for _ in range(H)]
    for (y0, x0), ids in zip(origins, np.asarray(frame_ids).tolist()):
        if y0 < 0 or x0 < 0 or y0 + 32 > H or x0 + 32 > W:
            continue
        if any(f < 0 or f >= T for f in ids):
            continue
        for f in ids:
            for y in range(y0, y0 + 32):
                row = px[f][y]
                for x in range(x0, x0 + 32):
                    r, g, b = row[x]
                    if r != 0 and g != 0 and b != 0:
                        sup[y][x] += 1
    return np.array(sup, np.int64)


def brute_apply(mosaic, support, m):
    out = mosaic.copy()
    Ho, Wo, C = mosaic.shape
    for y in range(Ho):
        for x in range(Wo):
            s = int(support[y // 4, x // 4])
            for c in range(C):
                out[y, x, c] = 0 if s < m else max(1, int(mosaic[y, x, c]))
    return out


def nodata_scene(seed, T=5, H=70, W=45):
    """zeros planted per byte (about 5 %), one column zero in every frame, one whole frame zero"""
    rng = np.random.RandomState(seed)
    tci = rng.randint(1, 256, size=(T, H, W, 3)).astype(np.uint8)
    tci[rng.rand(T, H, W, 3) < 0.05] = 0
    tci[:, :, 17] = 0
    tci[3] = 0
    return tci


def test_scene_support_equals_the_brute_force_count():
    from satlas_super_resolution_amd.infer_scene import scene_support
    T, H, W, n = 5, 70, 45, 3
    tci = nodata_scene(1, T, H, W)
    rng = np.random.RandomState(2)
    origins = [(0, 0), (38, 13), (37, 12), (H - 32, W - 32), (10, 5), (39, 0), (0, 14), (-1, 0), (3, 3)]
    ids = np.stack([rng.permutation(T)[:n] for _ in origins]).astype(np.int32)
    ids[4] = (2, 2, 0)                             # a frame in two slots counts twice
    ids[-1] = (0, T, 1)                            # a frame id outside the scene: the chunk contributes nothing
    want = brute_support(tci, origins, ids)
    got = scene_support(tci, origins, ids)
    assert got.dtype == np.int32 and got.shape == (H, W)
    assert np.array_equal(got, want)
    assert want.max() > n and (want[:, 17] == 0).all() and (want > 0).sum() > 1000
    # the chunks that contribute nothing really do: the same map without them
    assert np.array_equal(scene_support(tci, origins[:5], ids[:5]), want)
    ids_neg = ids[:5].copy()
    ids_neg[0, 1] = -1
    assert np.array_equal(scene_support(tci, origins[:5], ids_neg), brute_support(tci, origins[:5], ids_neg))
    assert not np.array_equal(scene_support(tci, origins[:5], ids_neg), want)
    assert not scene_support(tci, np.zeros((0, 2), np.int32), np.zeros((0, n), np.int32)).any()


def test_support_exceeds_n_under_the_triple_cover_at_an_axis_end():
    from satlas_super_resolution_amd.infer_scene import scene_chunk_origins, scene_support
    assert scene_chunk_origins(52, 16) == [0, 16, 20]
    T, H, W, n, overlap = 5, 70, 45, 3, 16
    assert scene_chunk_origins(H, overlap) == [0, 16, 32, 38] and scene_chunk_origins(W, overlap) == [0, 13]
    tci = nodata_scene(3, T, H, W)
    tci[:3, 40:46, 20:26] = 9                      # rows 38 .. 47 lie in three chunks, columns 13 .. 31 in two: all data here
    origins = grid_of(H, W, overlap)
    ids = np.tile(np.array([0, 1, 2], np.int32), (len(origins), 1))
    got = scene_support(tci, origins, ids)
    assert np.array_equal(got, brute_support(tci, origins, ids))
    assert (got[40:46, 20:26] == 3 * 2 * n).all() and got.max() == 6 * n and got.max() <= 9 * n
    # on the grid every pixel has one covering chunk: support <= n
    tci = nodata_scene(4, T, 64, 96)
    origins = grid_of(64, 96, 0)
    ids = np.tile(np.array([4, 0, 2], np.int32), (len(origins), 1))
    got = scene_support(tci, origins, ids)
    assert np.array_equal(got, brute_support(tci, origins, ids)) and got.max() == n


@pytest.mark.parametrize("C", [1, 3, 4])
def test_apply_nodata_equals_the_brute_force_rule(C):
    from satlas_super_resolution_amd.infer_scene import apply_nodata
    rng = np.random.RandomState(C)
    H, W = 9, 7
    support = rng.randint(0, 4, size=(H, W)).astype(np.int32)
    support[0, :4] = (254, 255, 256, 70000)
    mosaic = rng.randint(0, 256, size=(4 * H, 4 * W, C)).astype(np.uint8)
    mosaic[rng.rand(4 * H, 4 * W, C) < 0.2] = 0     # zeros inside supported pixels: they become 1
    for m in (1, 2, 3):
        got = apply_nodata(mosaic, support, m)
        assert got.dtype == np.uint8 and np.array_equal(got, brute_apply(mosaic, support, m)), m
        up = np.repeat(np.repeat(support, 4, 0), 4, 1)
        assert (got[up < m] == 0).all() and (got[up >= m] >= 1).all()
        keep = (up >= m)[:, :, None] & (mosaic > 0)
        assert np.array_equal(got[keep], mosaic[keep])                   # a sample above 0 of a supported pixel is untouched
        clamped = (up >= m)[:, :, None] & (mosaic == 0)
        assert clamped.sum() > 20 and (got[clamped] == 1).all()          # 0 -> 1: 0 stays reserved for NODATA
    assert np.array_equal(apply_nodata(mosaic, support), apply_nodata(mosaic, support, 1))
    with pytest.raises(ValueError, match="min_support"):
        apply_nodata(mosaic, support, 0)


def test_the_returned_support_map_saturates_at_255():
    from satlas_super_resolution_amd.infer_scene import support_to_u8
    got = support_to_u8(np.array([[0, 1, 254], [255, 256, 70000]], np.int32))
    assert got.dtype == np.uint8 and got.tolist() == [[0, 1, 254], [255, 255, 255]]


# ---------------------------------------------------------------- the option and its refusals
def test_nodata_values_are_checked_on_the_host():
    from satlas_super_resolution_amd.infer_scene import check_nodata
    assert check_nodata("fill") == ("fill", 1) and check_nodata("fill", 1) == ("fill", 1)
    assert check_nodata("keep") == ("keep", 1) and check_nodata("keep", 7) == ("keep", 7)
    assert check_nodata("keep", np.int64(2)) == ("keep", 2)
    for bad in ("mask", "", None, "Keep", 1, True):
        with pytest.raises(ValueError, match="nodata"):
            check_nodata(bad)
    for bad in (0, -1, 1.0, 2.5, "2", None, True):
        with pytest.raises(ValueError, match="min_support"):
            check_nodata("keep", bad)
    with pytest.raises(ValueError, match="min_support"):                 # a threshold without a support map
        check_nodata("fill", 2)


@pytest.mark.parametrize("blended", [False, True])
def test_scene_functions_refuse_before_touching_the_device(blended):
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene, super_resolve_scene_blended
    fn = super_resolve_scene_blended if blended else super_resolve_scene
    sig = inspect.signature(fn).parameters                                # `fill` is the default: absent means today's paths
    assert (sig["nodata"].default, sig["min_support"].default, sig["return_support"].default) == ("fill", 1, False)
    net = SSR_RRDBNet(num_in_ch=6, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8)
    frames = np.ones((3, 32, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="nodata"):
        fn(net, frames, 2, nodata="mask")
    with pytest.raises(ValueError, match="min_support"):
        fn(net, frames, 2, nodata="keep", min_support=0)
    with pytest.raises(ValueError, match="min_support"):
        fn(net, frames, 2, nodata="keep", min_support=1.5)
    with pytest.raises(ValueError, match="min_support"):
        fn(net, frames, 2, min_support=2)
    with pytest.raises(ValueError, match="return_support"):
        fn(net, frames, 2, return_support=True)
    with pytest.raises(ValueError, match="return_support"):
        fn(net, frames, 2, nodata="fill", return_support=True)


def test_driver_reads_nodata(tmp_path):
    import torch
    from satlas_super_resolution_amd.infer_scene import run_infer_scene
    missing = str(tmp_path / "not_there") + "/"
    opt = {"data_dir": missing, "save_path": str(tmp_path / "out") + "/", "n_lr_images": 2, "io_workers": 1}
    with pytest.raises(ValueError, match="nodata"):                      # before the weights or the scene folder are looked at
        run_infer_scene(dict(opt, nodata="drop"))
    with pytest.raises(ValueError, match="min_support"):
        run_infer_scene(dict(opt, nodata="keep", nodata_min_support=0))
    with pytest.raises(ValueError, match="min_support"):
        run_infer_scene(dict(opt, nodata_min_support=2))
    os.makedirs(tmp_path / "empty")
    opt["data_dir"] = str(tmp_path / "empty") + "/"
    res = run_infer_scene(dict(opt), model=object(), device=torch.device("cpu"))             # no scenes: nothing reaches a device
    assert sorted(res) == ["chunks", "frame_select", "io_workers", "scenes", "seconds"]      # the dictionary of today
    assert sorted(run_infer_scene(dict(opt, nodata="fill"), model=object(), device=torch.device("cpu"))) == sorted(res)
    res = run_infer_scene(dict(opt, nodata="keep", nodata_min_support=2), model=object(), device=torch.device("cpu"))
    assert (res["nodata"], res["nodata_min_support"], res["scenes"]) == ("keep", 2, 0)


def test_grayscale_png_round_trip():
    """the support map's file: 8-bit grayscale [H, W] through the driver's own encoder"""
    import io
    from PIL import Image
    from satlas_super_resolution_amd import png_io
    a = np.arange(33 * 35, dtype=np.int64).reshape(33, 35).astype(np.uint8)
    im = Image.open(io.BytesIO(png_io.encode_png(a)))
    assert im.mode == "L" and np.array_equal(np.asarray(im), a)


# ---------------------------------------------------------------- interface
def test_nodata_entry_points_are_declared():
    from satlas_super_resolution_amd import hip
    src = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in hip.ABI_SYMBOLS


def test_nodata_entry_points_refuse_bad_arguments_without_a_launch():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    p = 4096                                     # a non-null, aligned address: every call below returns before a launch
    assert lib.ssr_scene_support_add(p, 5, 31, 64, p, p, 1, 3, p, None) == -2                # smaller than a chunk
    assert lib.ssr_scene_support_add(p, 5, 64, 20, p, p, 1, 3, p, None) == -2
    assert lib.ssr_scene_support_add(p, 2, 40, 50, p, p, 1, 3, p, None) == -2                # n > T
    assert lib.ssr_scene_support_add(None, 5, 40, 50, p, p, 1, 3, p, None) == -1
    assert lib.ssr_scene_support_add(p, 5, 40, 50, None, p, 1, 3, p, None) == -1             # no origins
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, None, 1, 3, p, None) == -1             # no frame ids
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, p, 1, 3, None, None) == -1             # no support
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, p, 1, 3, p + 2, None) == -1            # support not 4-byte aligned
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, p, 0, 3, p, None) == -1
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, p, 1, 0, p, None) == -1
    assert lib.ssr_scene_support_add(p, 5, 40, 50, p, p, (1 << 20) + 1, 3, p, None) == -1
    assert lib.ssr_scene_apply_nodata(p, 130, 128, 3, p, 1, None, None) == -2                # no multiple of 4
    assert lib.ssr_scene_apply_nodata(p, 128, 126, 3, p, 1, None, None) == -2
    assert lib.ssr_scene_apply_nodata(None, 128, 128, 3, p, 1, None, None) == -1
    assert lib.ssr_scene_apply_nodata(p, 128, 128, 3, None, 1, None, None) == -1
    assert lib.ssr_scene_apply_nodata(p, 128, 128, 0, p, 1, None, None) == -1
    assert lib.ssr_scene_apply_nodata(p, 128, 128, 9, p, 1, None, None) == -1                # more than 8 channels
    assert lib.ssr_scene_apply_nodata(p, 128, 128, 3, p, 0, None, None) == -1                # min_support < 1
    assert lib.ssr_scene_apply_nodata(p + 1, 128, 128, 3, p, 1, None, None) == -1            # mosaic not 4-byte aligned
    assert lib.ssr_scene_apply_nodata(p, 128, 128, 3, p + 2, 1, None, None) == -1
    assert lib.ssr_abi_version() == 3
