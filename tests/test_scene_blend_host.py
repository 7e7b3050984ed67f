"""CPU: the host half of blended scene inference (satlas_super_resolution_amd/infer_scene.py) - where the overlapping chunks of a
scene of any size sit, the blend window and its sums, a numpy restatement of the integer blend (`blend_reference`, which
tests/test_gpu_scene_blend.py compares the kernels with, byte for byte) - and the declaration of the four device entry points."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = ("ssr_scene_zero_scan_at", "ssr_scene_gather_at", "ssr_scene_blend_add", "ssr_scene_blend_finish")


# ---------------------------------------------------------------- the definition, restated in numpy
def fixed_point(v):
    """(uint32) (fminf(fmaxf(v, 0), 1) * 65535.0f): the clamp sends NaN to 0, ONE fp32 multiply, truncation"""
    v = np.asarray(v, np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    p = c * np.float32(65535.0)
    assert p.dtype == np.float32
    return p.astype(np.uint32)


def blend_accumulate(chunk_outputs, origins, H, W, overlap):
    """chunk_outputs [N, 128, 128, C] (floats), origins N x (y0, x0) in low-resolution pixels -> the accumulator, uint32 [4H, 4W, C].
    Items whose origin lies outside the scene are skipped.  Summed in uint64 to check the 2^32 bound."""
    from satlas_super_resolution_amd.infer_scene import blend_window
    w = blend_window(overlap).astype(np.uint64)
    ww = (w[:, None] * w[None, :])[:, :, None]
    C = chunk_outputs.shape[-1]
    acc = np.zeros((4 * H, 4 * W, C), np.uint64)
    for out, (y0, x0) in zip(chunk_outputs, origins):
        if not (0 <= y0 <= H - 32 and 0 <= x0 <= W - 32):
            continue
        acc[4 * y0:4 * y0 + 128, 4 * x0:4 * x0 + 128] += fixed_point(out).astype(np.uint64) * ww
    assert int(acc.max()) < 2 ** 32
    return acc.astype(np.uint32)


def blend_finish(acc, H, W, overlap):
    from satlas_super_resolution_amd.infer_scene import blend_weight_sums
    Sy, Sx = blend_weight_sums(H, overlap).astype(np.uint64), blend_weight_sums(W, overlap).astype(np.uint64)
    den = Sy[:, None, None] * Sx[None, :, None] * np.uint64(65535)
    return (acc.astype(np.uint64) * np.uint64(255) // den).astype(np.uint8)


def blend_reference(chunk_outputs, origins, H, W, overlap):
    """the mosaic uint8 [4H, 4W, C] of chunk outputs [N, 128, 128, C] placed at `origins` in an H x W scene"""
    return blend_finish(blend_accumulate(chunk_outputs, origins, H, W, overlap), H, W, overlap)


def grid_of(H, W, overlap):
    from satlas_super_resolution_amd.infer_scene import scene_chunk_origins
    return [(y, x) for y in scene_chunk_origins(H, overlap) for x in scene_chunk_origins(W, overlap)]


# ---------------------------------------------------------------- layout
def test_chunk_origins_and_their_refusals():
    from satlas_super_resolution_amd.infer_scene import scene_chunk_grid, scene_chunk_origins
    assert scene_chunk_origins(64, 0) == [0, 32]
    assert scene_chunk_origins(72, 8) == [0, 24, 40]
    assert scene_chunk_origins(40, 8) == [0, 8]
    assert scene_chunk_origins(49, 16) == [0, 16, 17]
    assert scene_chunk_origins(32, 0) == [0] and scene_chunk_origins(32, 16) == [0] and scene_chunk_origins(33, 0) == [0, 1]
    assert scene_chunk_origins(512, 0) == list(range(0, 512, 32)) and len(scene_chunk_origins(512, 8)) == 21
    for bad in (-1, 17, 32, 2.5):
        with pytest.raises(ValueError, match="overlap"):
            scene_chunk_origins(64, bad)
    with pytest.raises(ValueError, match="31"):
        scene_chunk_origins(31, 8)
    with pytest.raises(ValueError, match="0"):
        scene_chunk_origins(0, 0)
    g = scene_chunk_grid(40, 72, 8)                                     # row-major cross product
    assert g.dtype == np.int32 and g.tolist() == [[0, 0], [0, 24], [0, 40], [8, 0], [8, 24], [8, 40]]


def test_every_pixel_is_covered_by_at_most_three_chunks_per_axis_and_the_accumulator_fits_32_bits():
    from satlas_super_resolution_amd.infer_scene import blend_weight_sums, blend_window, scene_chunk_origins
    worst_S, worst_cover = 0, 0
    for overlap in range(17):
        w = blend_window(overlap)
        for L in range(32, 260):
            org = scene_chunk_origins(L, overlap)
            assert org[0] == 0 and org[-1] == L - 32 and org == sorted(set(org)), (L, overlap, org)
            cover = np.zeros(L, int)
            S = np.zeros(4 * L, np.int64)
            for o in org:
                cover[o:o + 32] += 1
                S[4 * o:4 * o + 128] += w
            assert cover.min() >= 1 and cover.max() <= 3, (L, overlap, org)
            assert np.array_equal(blend_weight_sums(L, overlap), S) and S.min() >= 1
            worst_S, worst_cover = max(worst_S, int(S.max())), max(worst_cover, int(cover.max()))
    print(f"largest weight sum per axis {worst_S}, largest cover per axis {worst_cover}")
    assert worst_S <= 125 and worst_cover == 3
    assert worst_S ** 2 * 65535 < 2 ** 32                                # every sample 1.0 everywhere: the largest accumulator word


def test_blend_window_and_weight_sums():
    from satlas_super_resolution_amd.infer_scene import blend_weight_sums, blend_window
    w = blend_window(8)
    assert w.dtype == np.int32 and w.shape == (128,)
    assert w[:33].tolist() == list(range(1, 33)) + [32] and w[95:].tolist() == [32] + list(range(32, 0, -1))
    assert (w[32:96] == 32).all() and np.array_equal(w, w[::-1])
    assert (blend_window(0) == 1).all()                                  # R = 1: a plain paste
    assert blend_window(16).max() == 64 and blend_window(1).tolist()[:5] == [1, 2, 3, 4, 4]
    for r in range(128):
        assert blend_window(5)[r] == min(r + 1, 128 - r, 20)
    with pytest.raises(ValueError):
        blend_window(17)
    S = blend_weight_sums(72, 8)                                         # chunks at 0, 24, 40: a regular overlap, then an irregular one
    assert S.dtype == np.int32 and S.shape == (288,)
    assert S[:96].tolist() == w[:96].tolist()                            # one chunk only
    assert (S[96:128] == 33).all()                                       # two ramps of a regular overlap zone: R + 1, a linear cross-fade
    assert (S[128:160] == 32).all() and S[287] == 1 and S[160] == 32 + 1
    assert (blend_weight_sums(64, 0) == 1).all()


# ---------------------------------------------------------------- the blend
def test_a_constant_input_comes_out_as_the_same_constant():
    H, W, overlap = 49, 50, 16                                           # 9 chunks, 9-fold cover in the middle
    org = grid_of(H, W, overlap)
    assert len(org) == 9
    for v in (0.0, 0.3, 0.5, 200 / 255, 1.0, 1.7, -0.2):
        outs = np.full((9, 128, 128, 3), v, np.float32)
        got = blend_reference(outs, org, H, W, overlap)
        want = int(fixed_point(v)) * 255 // 65535
        assert got.shape == (196, 200, 3) and (got == want).all(), v
    assert int(fixed_point(1.0)) * 255 // 65535 == 255 and int(fixed_point(0.5)) * 255 // 65535 == 127


def test_two_constant_chunks_cross_fade_monotonically():
    H, W, overlap = 32, 56, 8
    org = grid_of(H, W, overlap)
    assert org == [(0, 0), (0, 24)]
    a, b = 0.2, 0.9
    outs = np.stack([np.full((128, 128, 3), a, np.float32), np.full((128, 128, 3), b, np.float32)])
    got = blend_reference(outs, org, H, W, overlap)
    qa, qb = int(fixed_point(a)) * 255 // 65535, int(fixed_point(b)) * 255 // 65535
    assert (got[:, :96] == qa).all() and (got[:, 128:] == qb).all()
    ramp = got[:, 96:128].astype(int)
    assert (ramp == ramp[:1]).all() and (ramp[..., 0] == ramp[..., 2]).all()         # the same in every row and channel
    d = np.diff(ramp[0, :, 0])
    assert (d >= 0).all() and d.max() <= (qb - qa) // 32 + 1                          # monotone and linear: steps of (qb - qa) / 33
    assert qa < ramp[0, 0, 0] < ramp[0, -1, 0] < qb
    flipped = blend_reference(outs[::-1], org, H, W, overlap)
    assert (np.diff(flipped[5, 96:128, 1].astype(int)) <= 0).all()


def test_without_overlap_the_blend_is_the_truncating_quantiser_pasted():
    H, W = 64, 96
    org = grid_of(H, W, 0)
    assert org == [(i, j) for i in (0, 32) for j in (0, 32, 64)]
    rng = np.random.RandomState(4)
    outs = (rng.rand(6, 128, 128, 3) * 1.4 - 0.2).astype(np.float32)
    k = rng.randint(0, 256, size=(6, 128, 16, 3)).astype(np.float32) / np.float32(255)   # at, just above and just below k / 255
    outs[:, :, :16] = k
    outs[:, :, 16:32] = np.nextafter(k, np.float32(2))
    outs[:, :, 32:48] = np.nextafter(k, np.float32(-1))
    outs[0, 0, 0] = [0.0, 1.0, np.nan]
    want = np.zeros((256, 384, 3), np.uint8)
    q = (np.where(np.isnan(outs), np.float32(0), np.clip(outs, 0, 1)).astype(np.float32) * np.float32(255.0)).astype(np.uint8)
    for cell, (y0, x0) in zip(q, org):
        want[4 * y0:4 * y0 + 128, 4 * x0:4 * x0 + 128] = cell
    got = blend_reference(outs, org, H, W, 0)
    print(f"differing samples {int((got != want).sum())} of {got.size}")
    assert np.array_equal(got, want)
    assert len(np.unique(got)) == 256


# ---------------------------------------------------------------- interface
def test_parse_scene_takes_any_size_only_when_asked():
    from satlas_super_resolution_amd.infer_scene import parse_scene
    a = np.ones((2, 40, 50, 3), np.uint8)
    assert parse_scene(a, any_size=True).shape == (2, 40, 50, 3)
    assert parse_scene(a.reshape(80, 50, 3), scene_hw=[40, 50], any_size=True).shape == (2, 40, 50, 3)
    with pytest.raises(ValueError, match="40 x 50"):
        parse_scene(a)
    with pytest.raises(ValueError, match="40 x 50"):
        parse_scene(a, any_size=False)
    with pytest.raises(ValueError, match="31 x 50"):
        parse_scene(np.ones((2, 31, 50, 3), np.uint8), any_size=True)
    with pytest.raises(ValueError, match="64 x 20"):
        parse_scene(np.ones((1, 64, 20, 3), np.uint8), any_size=True)


def test_blended_scene_refusals_come_before_the_device_is_touched():
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene_blended
    net = SSR_RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8)
    with pytest.raises(ValueError, match="31 x 64"):
        super_resolve_scene_blended(net, np.ones((1, 31, 64, 3), np.uint8), 1)
    with pytest.raises(ValueError, match="overlap"):
        super_resolve_scene_blended(net, np.ones((1, 40, 64, 3), np.uint8), 1, overlap=17)
    net2 = SSR_RRDBNet(num_in_ch=3, num_out_ch=3, scale=2, num_feat=16, num_block=1, num_grow_ch=8)
    with pytest.raises(NotImplementedError, match="scale"):
        super_resolve_scene_blended(net2, np.ones((1, 40, 64, 3), np.uint8), 1)


def test_blend_entry_points_are_declared():
    from satlas_super_resolution_amd import hip
    src = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in hip.ABI_SYMBOLS


def test_blend_entry_points_refuse_bad_geometry_without_a_launch():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    p = 4096                                     # a non-null, 16-byte aligned address: every call below returns before a launch
    v = hip.View(p, 8, 0)
    assert lib.ssr_scene_zero_scan_at(p, 2, 31, 64, p, 1, p, None) == -2                     # smaller than a chunk
    assert lib.ssr_scene_zero_scan_at(p, 2, 64, 20, p, 1, p, None) == -2
    assert lib.ssr_scene_zero_scan_at(None, 2, 40, 50, p, 1, p, None) == -1
    assert lib.ssr_scene_zero_scan_at(p, 2, 40, 50, None, 1, p, None) == -1                  # no origins
    assert lib.ssr_scene_zero_scan_at(p, 2, 40, 50, p, 0, p, None) == -1
    assert lib.ssr_scene_gather_at(p, 2, 64, 20, p, p, 1, 1, v, hip.F32, None) == -2
    assert lib.ssr_scene_gather_at(p, 2, 40, 50, p, p, 1, 3, hip.View(p, 16, 0), hip.F32, None) == -2      # n > T
    assert lib.ssr_scene_gather_at(p, 2, 40, 50, p, p, 1, 1, v, 7, None) == -2               # a dtype the converters do not know
    assert lib.ssr_scene_gather_at(p, 2, 40, 50, p, p, 1, 1, v, hip.F32H3, None) == -2
    assert lib.ssr_scene_gather_at(p, 4, 40, 50, p, p, 1, 3, v, hip.F32, None) == -1         # 9 channels do not fit a pixel of 8
    assert lib.ssr_scene_gather_at(p, 2, 40, 50, None, p, 1, 1, v, hip.F32, None) == -1
    # an invalid argument beside an unsupported shape: the invalid argument wins
    assert lib.ssr_scene_gather_at(p, 2, 64, 20, None, p, 1, 1, v, hip.F32, None) == -1      # no origins, narrower than a chunk
    assert lib.ssr_scene_gather_at(p, 4, 64, 20, p, p, 1, 3, v, 7, None) == -1               # 9 channels in a pixel of 8, W and dtype
    assert lib.ssr_scene_blend_add(v, 7, p, 1, 3, p, p, 160, 200, p, None) == -2
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, p, p, 160, 202, p, None) == -2       # not 4 x a width
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, p, p, 124, 200, p, None) == -2       # lower than a chunk
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, p, p, 160, 200, None, None) == -1    # no counter
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, None, p, 160, 200, p, None) == -1    # no window
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, p, p + 4, 160, 200, p, None) == -1   # accumulator not 16-byte aligned
    assert lib.ssr_scene_blend_add(hip.View(p, 16, 0), hip.F32, p, 1, 9, p, p, 160, 200, p, None) == -1    # more than 8 channels
    assert lib.ssr_scene_blend_add(hip.View(p, 8, 8), hip.F32, p, 1, 3, p, p, 160, 200, p, None) == -1     # channels outside the pixel
    assert lib.ssr_scene_blend_add(v, 7, p, 1, 3, p, p, 160, 202, None, None) == -1          # no counter, an unknown dtype and width
    assert lib.ssr_scene_blend_add(v, hip.F32, p, 1, 3, p, p + 4, 124, 200, p, None) == -1   # accumulator alignment, lower than a chunk
    assert lib.ssr_scene_blend_finish(p, p, p, 3, p, 160, 202, None) == -2
    assert lib.ssr_scene_blend_finish(p, p, p, 3, p, 100, 200, None) == -2
    assert lib.ssr_scene_blend_finish(p, None, p, 3, p, 160, 200, None) == -1
    assert lib.ssr_scene_blend_finish(p, p, p, 3, p + 2, 160, 200, None) == -1               # mosaic not 4-byte aligned
    assert lib.ssr_scene_blend_finish(p, p, p, 9, p, 160, 200, None) == -1
    assert lib.ssr_scene_blend_finish(p, None, p, 3, p, 160, 202, None) == -1                # no row sums, not 4 x a width
    assert lib.ssr_scene_blend_finish(p, p, p, 9, p, 100, 200, None) == -1                   # 9 channels, lower than a chunk
    assert lib.ssr_abi_version() == 3
