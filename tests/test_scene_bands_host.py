"""CPU: the host half of multi-band scene inference (satlas_super_resolution_amd/infer_scene.py, `s2_bands`) - the listing of scene
directories, the checks of the band files and of the `bands` argument, and the declaration and refusals of the device entry point
ssr_scene_gather_bands."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

S2 = os.path.join(GOLDEN, "s2naip_mini", "sentinel2")


def test_band_scenes_are_listed_by_name_with_missing_band_files_marked():
    from satlas_super_resolution_amd.infer_scene import list_band_scenes
    scenes = list_band_scenes(S2, ["tci", "b08"])
    assert [s[0] for s in scenes] == ["100_200", "100_201", "101_200", "101_201", "102_200"]
    for name, tci, bands in scenes:
        assert tci == os.path.join(S2, name, "tci.png") and len(bands) == 1
        assert bands[0] == (None if name == "101_201" else os.path.join(S2, name, "b08.png")), name
    # tci goes first wherever it stands, the other bands keep their order; a band without any file is missing everywhere
    scenes = list_band_scenes(S2, ["b08", "tci", "b05"])
    assert [os.path.basename(p) if p else None for p in scenes[0][2]] == ["b08.png", None]
    assert all(s[2][1] is None for s in scenes)
    assert [s[2] for s in list_band_scenes(S2, ["tci"])] == [[]] * 5


def test_a_band_list_without_tci_is_refused():
    from satlas_super_resolution_amd.infer_scene import list_band_scenes, order_s2_bands
    assert order_s2_bands(["b05", "tci", "b08"]) == ["tci", "b05", "b08"]          # the dataset's order
    with pytest.raises(ValueError, match="tci"):
        list_band_scenes(S2, ["b08"])
    with pytest.raises(ValueError, match="tci"):
        order_s2_bands([])


def test_a_band_file_of_another_size_or_mode_is_refused_by_name(tmp_path):
    from PIL import Image
    from satlas_super_resolution_amd.infer_scene import band_scene_shape, list_band_scenes
    d = tmp_path / "t"
    os.makedirs(d)
    rng = np.random.RandomState(0)
    Image.fromarray(rng.randint(0, 256, size=(128, 64, 3)).astype(np.uint8)).save(d / "tci.png")
    Image.fromarray(rng.randint(0, 256, size=(128, 64)).astype(np.uint8)).save(d / "b05.png")
    Image.fromarray(rng.randint(0, 256, size=(128, 32)).astype(np.uint8)).save(d / "b08.png")          # half the width
    Image.fromarray(rng.randint(0, 256, size=(64, 64)).astype(np.uint8)).save(d / "b11.png")           # half the rows
    Image.fromarray(rng.randint(0, 256, size=(128, 64, 3)).astype(np.uint8)).save(d / "b12.png")       # RGB
    Image.fromarray(rng.randint(0, 60000, size=(128, 64)).astype(np.uint16)).save(d / "b01.png")       # 16-bit grayscale

    def shape_of(bands):
        (name, tci, paths), = list_band_scenes(str(tmp_path), bands)
        return band_scene_shape(tci, paths)

    assert shape_of(["tci", "b05"]) == (128, 64)
    assert shape_of(["tci", "b05", "b09"]) == (128, 64)                              # a missing file is no error: zeros
    for bad in ("b08", "b11", "b12", "b01"):
        with pytest.raises(ValueError, match=bad + r"\.png"):
            shape_of(["tci", "b05", bad])
    # the workers' decoder refuses the same files, should one change between the check and the decode
    from satlas_super_resolution_amd import png_io
    blk = png_io.ShmBlock(128 * 64, str(tmp_path), "x")
    try:
        for bad in ("b08", "b12", "b01"):
            with pytest.raises(ValueError, match=bad + r"\.png"):
                png_io.read_gray_into(str(d / (bad + ".png")), blk.path, blk.nbytes, 0, (128, 64), True)
        assert png_io.read_gray_into(str(d / "b05.png"), blk.path, blk.nbytes, 0, (128, 64), True) == (128, 64)
        assert np.array_equal(blk.buf.reshape(128, 64), np.asarray(Image.open(d / "b05.png")))
    finally:
        blk.close()


def _net(c_in):
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    return SSR_RRDBNet(num_in_ch=c_in, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8)


@pytest.mark.parametrize("blended", [False, True])
def test_the_bands_argument_is_checked_before_the_device_is_touched(blended):
    """the generators live on the CPU here: anything that got past the checks would fail in another way"""
    from satlas_super_resolution_amd import infer_scene as S
    run = S.super_resolve_scene_blended if blended else S.super_resolve_scene
    frames = np.ones((4, 64, 96, 3), np.uint8)
    bands = np.ones((2, 4, 64, 96), np.uint8)
    with pytest.raises(ValueError, match=r"10.*6|6.*10"):                           # 2 (3 + 2) = 10 channels into a generator of 6
        run(_net(6), frames, 2, bands=bands)
    with pytest.raises(ValueError, match=r"5.*10|10.*5"):                           # n = 1: 5 channels into a generator of 10
        run(_net(10), frames, 1, bands=bands)
    net = _net(10)
    with pytest.raises(ValueError, match=r"K, T, H, W"):                             # rank
        run(net, frames, 2, bands=bands[0])
    with pytest.raises(ValueError, match=r"K, T, H, W"):
        run(net, frames, 2, bands=bands[..., None])
    with pytest.raises(ValueError, match="float32"):                                 # dtype
        run(net, frames, 2, bands=bands.astype(np.float32))
    with pytest.raises(ValueError, match="float32"):
        run(net, frames, 2, bands=torch.ones(2, 4, 64, 96))
    for shape in ((2, 3, 64, 96), (2, 4, 32, 96), (2, 4, 64, 64)):                   # T, H, W
        with pytest.raises(ValueError, match=re.escape(str(shape[1:])) + ".*" + re.escape("(4, 64, 96)")):
            run(net, frames, 2, bands=np.ones(shape, np.uint8))
    with pytest.raises(ValueError, match=r"K, T, H, W"):                             # no band at all
        run(net, frames, 2, bands=np.ones((0, 4, 64, 96), np.uint8))
    with pytest.raises(ValueError, match="6 input channels"):                        # without bands: today's refusal
        run(net, frames, 2)


def test_the_entry_point_is_declared_and_bound():
    from satlas_super_resolution_amd import hip
    src = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ssr_scene_gather_bands\s*\(", src)
    assert "ssr_scene_gather_bands" in hip.ABI_SYMBOLS


def test_the_entry_point_refuses_bad_arguments_without_a_launch():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    p = 4096                                     # a non-null, 16-byte aligned address: every call below returns before a launch
    v = hip.View(p, 8, 0)
    g = lib.ssr_scene_gather_bands
    assert g(None, p, 1, 2, 40, 50, p, p, 1, 1, v, hip.F32, None) == -1             # null pointers
    assert g(p, None, 1, 2, 40, 50, p, p, 1, 1, v, hip.F32, None) == -1
    assert g(p, p, 1, 2, 40, 50, None, p, 1, 1, v, hip.F32, None) == -1
    assert g(p, p, 1, 2, 40, 50, p, None, 1, 1, v, hip.F32, None) == -1
    assert g(p, p, 1, 2, 40, 50, p, p, 1, 1, hip.View(None, 8, 0), hip.F32, None) == -1
    assert g(p, p, 0, 2, 40, 50, p, p, 1, 1, v, hip.F32, None) == -1                # K < 1
    assert g(p, p, -1, 2, 40, 50, p, p, 1, 1, v, hip.F32, None) == -1
    assert g(p, p, 6, 2, 40, 50, p, p, 1, 1, v, hip.F32, None) == -1                # 9 channels do not fit a pixel of 8
    assert g(p, p, 1, 4, 40, 50, p, p, 1, 3, v, hip.F32, None) == -1                # 12 channels do not fit a pixel of 8
    assert g(p, p, 1, 2, 40, 50, p, p, 1, 2, hip.View(p, 16, 16), hip.F32, None) == -1            # channels outside the pixel
    assert g(p, p, 1, 2, 40, 50, p, p, 1, 3, hip.View(p, 16, 0), hip.F32, None) == -2             # n > T
    assert g(p, p, 1, 2, 31, 64, p, p, 1, 1, v, hip.F32, None) == -2                # smaller than a chunk
    assert g(p, p, 1, 2, 64, 20, p, p, 1, 1, v, hip.F32, None) == -2
    assert g(p, p, 1, 2, 40, 50, p, p, 1, 1, v, 7, None) == -2                      # a dtype the converters do not know
    assert g(p, p, 1, 2, 40, 50, p, p, 1, 1, v, hip.F32H3, None) == -2
    # an invalid argument beside an unsupported shape: the invalid argument wins
    assert g(p, None, 1, 2, 64, 20, p, p, 1, 1, v, hip.F32, None) == -1             # no bands, narrower than a chunk
    assert g(p, p, 0, 2, 40, 50, p, p, 1, 3, v, 7, None) == -1                      # K < 1, n > T and an unknown dtype
    assert g(p, p, 1, 2, 64, 20, None, p, 1, 1, v, hip.F32, None) == -1             # no origins, narrower than a chunk
    assert g(p, p, 1, 4, 64, 20, p, p, 1, 3, v, hip.F32, None) == -1                # 12 channels in a pixel of 8, narrower than a chunk
    assert lib.ssr_abi_version() == 3
