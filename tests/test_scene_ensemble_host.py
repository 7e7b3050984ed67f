"""CPU: the host half of the self-ensemble of scene inference (satlas_super_resolution_amd/infer_scene.py, `self_ensemble`) - the two
numpy statements of the eight transforms (`ensemble_transform`, `ensemble_inverse`), why the accumulator carries 13 fractional bits, a
numpy restatement of the integer average (`ensemble_accumulate`, `ensemble_finish`, which tests/test_gpu_scene_ensemble.py compares the
kernels with, word for word and byte for byte), the refusals, and the declaration of the three device entry points."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_scene_blend_host import grid_of

ENTRIES = ("ssr_scene_gather_tf", "ssr_scene_blend_add_tf", "ssr_scene_blend_finish_scaled")


# ---------------------------------------------------------------- the definition, restated in numpy
def ensemble_fixed_point(v):
    """(uint32) (fminf(fmaxf(v, 0), 1) * 8191.0f): the clamp sends NaN to 0, ONE fp32 multiply, truncation"""
    v = np.asarray(v, np.float32)
    c = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(1))).astype(np.float32)
    p = c * np.float32(8191.0)
    assert p.dtype == np.float32
    return p.astype(np.uint32)


def ensemble_accumulate(row_outputs, row_origins, row_tf, H, W, overlap):
    """row_outputs [N, 128, 128, C] (floats: the generator's outputs of the rows), row_origins N x (y0, x0) in low-resolution
    pixels, row_tf N transform ids -> the accumulator, uint32 [4H, 4W, C]: every row's output turned back, in 13-bit fixed point,
    times the window.  Rows whose origin lies outside the scene or whose tf lies outside 0 .. 7 are skipped.  Summed in uint64 to
    check the 2^32 bound."""
    from satlas_super_resolution_amd.infer_scene import blend_window, ensemble_inverse
    w = blend_window(overlap).astype(np.uint64)
    ww = (w[:, None] * w[None, :])[:, :, None]
    C = row_outputs.shape[-1]
    acc = np.zeros((4 * H, 4 * W, C), np.uint64)
    for out, (y0, x0), tf in zip(row_outputs, row_origins, row_tf):
        if not (0 <= y0 <= H - 32 and 0 <= x0 <= W - 32) or not 0 <= tf <= 7:
            continue
        acc[4 * y0:4 * y0 + 128, 4 * x0:4 * x0 + 128] += ensemble_fixed_point(ensemble_inverse(out, tf)).astype(np.uint64) * ww
    assert int(acc.max()) < 2 ** 32
    return acc.astype(np.uint32)


def ensemble_finish(acc, H, W, overlap):
    from satlas_super_resolution_amd.infer_scene import blend_weight_sums
    Sy, Sx = blend_weight_sums(H, overlap).astype(np.uint64), blend_weight_sums(W, overlap).astype(np.uint64)
    den = np.uint64(8) * Sy[:, None, None] * Sx[None, :, None] * np.uint64(8191)
    return (acc.astype(np.uint64) * np.uint64(255) // den).astype(np.uint8)


def ensemble_rows(origins):
    """the generator's rows of the chunks at `origins`: (row origins, row transform ids), chunk-major with tf 0 .. 7 inside a chunk"""
    return [o for o in origins for _ in range(8)], [tf for _ in origins for tf in range(8)]


# ---------------------------------------------------------------- 1. the two functions
def _asym(h=5, w=5):
    return np.arange(h * w * 2).reshape(h, w, 2)                          # every entry its own value: no symmetry at all


def test_the_eight_transforms_are_distinct_and_spelled_as_the_three_bits():
    from satlas_super_resolution_amd.infer_scene import ENSEMBLE, ensemble_transform
    P = _asym()
    assert ENSEMBLE == 8
    got = [ensemble_transform(P, tf) for tf in range(8)]
    assert len({g.tobytes() for g in got}) == 8
    assert np.array_equal(got[0], P) and np.array_equal(got[1], P[:, ::-1]) and np.array_equal(got[2], P[::-1])
    assert np.array_equal(got[3], P[::-1, ::-1]) and np.array_equal(got[4], P.swapaxes(0, 1))
    assert np.array_equal(got[5], P[:, ::-1].swapaxes(0, 1)) and np.array_equal(got[7], P[::-1, ::-1].swapaxes(0, 1))
    for g in got:                                                         # the channel axis is untouched
        assert np.array_equal(np.sort(g.reshape(-1, 2), axis=0), np.sort(P.reshape(-1, 2), axis=0))
        assert (g[..., 1] - g[..., 0] == 1).all()
    Q = np.arange(3 * 5).reshape(3, 5)                                    # not square: a transpose swaps the two lengths
    assert ensemble_transform(Q, 6).shape == (5, 3) and ensemble_transform(Q, 3).shape == (3, 5)
    for bad in (-1, 8, 9):
        with pytest.raises(ValueError, match="tf"):
            ensemble_transform(P, bad)


def test_the_inverse_undoes_every_transform():
    from satlas_super_resolution_amd.infer_scene import ensemble_inverse, ensemble_transform
    P = _asym(4, 7)
    for tf in range(8):
        assert np.array_equal(ensemble_inverse(ensemble_transform(P, tf), tf), P), tf
        assert np.array_equal(ensemble_transform(ensemble_inverse(P, tf), tf), P), tf
    with pytest.raises(ValueError, match="tf"):
        ensemble_inverse(P, 8)
    # 5 (flip the columns, then transpose: a quarter turn) is not its own inverse: the inverse is not the transform again
    S = _asym()
    assert not np.array_equal(ensemble_transform(ensemble_transform(S, 5), 5), S)


def test_the_set_is_closed_under_each_of_the_eight_symmetries():
    from satlas_super_resolution_amd.infer_scene import ensemble_transform
    P = _asym()
    members = {ensemble_transform(P, tf).tobytes() for tf in range(8)}
    for g in range(8):
        after = {ensemble_transform(ensemble_transform(P, g), tf).tobytes() for tf in range(8)}
        assert after == members, g                                        # tf o g runs through the same eight: a group
        before = {ensemble_transform(ensemble_transform(P, tf), g).tobytes() for tf in range(8)}
        assert before == members, g


def test_an_output_turned_back_lands_on_the_4x_positions_of_its_chunk():
    from satlas_super_resolution_amd.infer_scene import ensemble_inverse, ensemble_transform
    ids = np.arange(32 * 32).reshape(32, 32)                              # the chunk's pixels by name
    sub = np.arange(16).reshape(4, 4)

    def upscale(A):
        """a stand-in generator that commutes with nothing: output pixel (4y + i, 4x + j) of input pixel A[y, x] is named
        (A[y, x], i, j) - the place inside the 4 x 4 block is recorded in the output's own frame"""
        return np.stack([np.repeat(np.repeat(A, 4, axis=0), 4, axis=1), np.tile(sub, A.shape)], axis=-1)

    home = upscale(ids)[..., 0]
    for tf in range(8):
        back = ensemble_inverse(upscale(ensemble_transform(ids, tf)), tf)
        assert back.shape == (128, 128, 2)
        assert np.array_equal(back[..., 0], home), tf                     # every sample over the low-resolution pixel it came from
        # inside the block the same transform has been undone: the block's own frame is the output's, turned back
        assert np.array_equal(back[..., 1], np.tile(ensemble_inverse(sub, tf), (32, 32))), tf


# ---------------------------------------------------------------- 2. why 13 fractional bits
def test_eight_rows_per_chunk_fit_32_bits_at_13_fractional_bits_and_not_at_16():
    from satlas_super_resolution_amd.infer_scene import ENSEMBLE, ENSEMBLE_ONE, blend_weight_sums
    assert (ENSEMBLE, ENSEMBLE_ONE) == (8, 8191)
    worst = 0
    for overlap in range(17):
        for L in range(32, 260):
            S = int(blend_weight_sums(L, overlap).max())
            assert 8 * S * S * 8191 < 2 ** 32, (overlap, L)
            worst = max(worst, S)
    print(f"largest weight sum per axis {worst}: 8 S^2 8191 = {8 * worst * worst * 8191 / 2 ** 32:.4f} x 2^32, "
          f"8 S^2 65535 = {8 * worst * worst * 65535 / 2 ** 32:.4f} x 2^32")
    assert worst == 125
    assert not 8 * worst * worst * 65535 < 2 ** 32                        # the existing 16 fractional bits would not fit
    assert 8 * worst * worst * 8191 < worst * worst * 65535               # and the words stay below the plain blend's largest
    assert 8 * 8191 < 2 ** 31                                             # (the finish's scale is an int32)


# ---------------------------------------------------------------- 3. the restatement
def test_all_ones_come_out_as_255_and_all_zeros_as_0():
    H, W, overlap = 49, 50, 16
    org, tf = ensemble_rows(grid_of(H, W, overlap))
    assert len(org) == 72 and tf[:9] == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    ones = ensemble_accumulate(np.ones((72, 128, 128, 3), np.float32), org, tf, H, W, overlap)
    assert int(ones.max()) > 2 ** 29
    assert (ensemble_finish(ones, H, W, overlap) == 255).all()
    zeros = ensemble_accumulate(np.zeros((72, 128, 128, 3), np.float32), org, tf, H, W, overlap)
    assert not zeros.any() and not ensemble_finish(zeros, H, W, overlap).any()
    for v, want in ((0.5, 127), (200 / 255, 199), (1.7, 255), (-0.2, 0), (np.nan, 0)):
        got = ensemble_finish(ensemble_accumulate(np.full((72, 128, 128, 3), v, np.float32), org, tf, H, W, overlap), H, W, overlap)
        assert (got == int(ensemble_fixed_point(v)) * 255 // 8191).all() and int(got[0, 0, 0]) == want, v


def test_the_restatement_averages_the_outputs_turned_back_and_skips_what_the_kernels_skip():
    H, W, overlap = 32, 56, 8
    origins = grid_of(H, W, overlap)
    assert origins == [(0, 0), (0, 24)]
    org, tf = ensemble_rows(origins)
    rng = np.random.RandomState(3)
    img = rng.rand(2, 128, 128, 3).astype(np.float32)
    from satlas_super_resolution_amd.infer_scene import ensemble_transform
    # a generator that commutes with the symmetries: every row's output is the transform of the same image
    outs = np.stack([ensemble_transform(img[k // 8], t) for k, t in enumerate(tf)])
    acc = ensemble_accumulate(outs, org, tf, H, W, overlap)
    one = ensemble_accumulate(outs[::8], origins, [0, 0], H, W, overlap)
    assert np.array_equal(acc, one * np.uint32(8))                        # eight equal terms
    got = ensemble_finish(acc, H, W, overlap)
    assert np.array_equal(got[:, :96], (ensemble_fixed_point(img[0, :, :96]) * 255 // 8191).astype(np.uint8))
    # rows the kernels skip: an origin outside the scene, a transform id outside 0 .. 7
    more = ensemble_accumulate(np.concatenate([outs, outs[:2]]), org + [(1, 0), (0, 0)], tf + [0, 9], H, W, overlap)
    assert np.array_equal(more, acc)


# ---------------------------------------------------------------- 4. the refusals
def test_self_ensemble_refusals_come_before_the_device_is_touched(tmp_path):
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.infer_scene import (check_self_ensemble, run_infer_scene, super_resolve_scene,
                                                         super_resolve_scene_blended)
    assert check_self_ensemble(True) is True and check_self_ensemble(False) is False and check_self_ensemble(np.bool_(True)) is True
    net = SSR_RRDBNet(num_in_ch=3, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8)
    good = np.ones((1, 64, 32, 3), np.uint8)
    for bad in (1, 0, "true", None, 8, [True]):
        with pytest.raises(ValueError, match="self_ensemble"):
            check_self_ensemble(bad)
        with pytest.raises(ValueError, match="self_ensemble"):
            super_resolve_scene(net, good, 1, self_ensemble=bad)
        with pytest.raises(ValueError, match="self_ensemble"):
            super_resolve_scene_blended(net, good, 1, self_ensemble=bad)
    # the grid entry point keeps its own refusal of sizes that are no multiples of 32; the blended one takes them
    with pytest.raises(ValueError, match="40 x 64.*multiples of 32"):
        super_resolve_scene(net, np.ones((1, 40, 64, 3), np.uint8), 1, self_ensemble=True)
    with pytest.raises(ValueError, match="31 x 64"):
        super_resolve_scene_blended(net, np.ones((1, 31, 64, 3), np.uint8), 1, self_ensemble=True)
    with pytest.raises(ValueError, match="overlap"):
        super_resolve_scene_blended(net, np.ones((1, 40, 64, 3), np.uint8), 1, overlap=17, self_ensemble=True)
    with pytest.raises(ValueError, match="input channels"):
        super_resolve_scene(net, np.ones((2, 64, 32, 3), np.uint8), 2, self_ensemble=True)
    with pytest.raises(ValueError, match="self_ensemble"):               # the driver's key: before a model is loaded
        run_infer_scene({"data_dir": str(tmp_path), "save_path": str(tmp_path / "out"), "n_lr_images": 1, "self_ensemble": "yes"})
    assert not os.path.exists(tmp_path / "out")


# ---------------------------------------------------------------- 5. the entry points
def test_ensemble_entry_points_are_declared():
    from satlas_super_resolution_amd import hip
    src = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in hip.ABI_SYMBOLS


def test_ensemble_entry_points_refuse_bad_geometry_without_a_launch():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    p = 4096                                     # a non-null, 16-byte aligned address: every call below returns before a launch
    v = hip.View(p, 8, 0)
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 64, 20, p, p, p, 1, 1, v, hip.F32, None) == -2          # smaller than a chunk
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 40, 50, p, p, p, 1, 3, hip.View(p, 16, 0), hip.F32, None) == -2      # n > T
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 40, 50, p, p, p, 1, 1, v, 7, None) == -2                # an unknown dtype
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 40, 50, p, p, None, 1, 1, v, hip.F32, None) == -1       # no transform ids
    assert lib.ssr_scene_gather_tf(p, None, 1, 2, 40, 50, p, p, p, 1, 1, v, hip.F32, None) == -1          # a band count without bands
    assert lib.ssr_scene_gather_tf(p, p, -1, 2, 40, 50, p, p, p, 1, 1, v, hip.F32, None) == -1
    assert lib.ssr_scene_gather_tf(p, p, 2, 4, 40, 50, p, p, p, 1, 2, v, hip.F32, None) == -1             # 10 channels, a pixel of 8
    assert lib.ssr_scene_gather_tf(p, None, 0, 4, 40, 50, p, p, p, 1, 3, v, hip.F32, None) == -1          # 9 channels, a pixel of 8
    assert lib.ssr_scene_gather_tf(None, None, 0, 2, 40, 50, p, p, p, 1, 1, v, hip.F32, None) == -1
    # an invalid argument beside an unsupported shape: the invalid argument wins
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 64, 20, p, p, None, 1, 1, v, hip.F32, None) == -1       # no transform ids, W < 32
    assert lib.ssr_scene_gather_tf(p, None, 1, 2, 40, 50, p, p, p, 1, 3, v, 7, None) == -1                # K without bands, n > T, dtype
    assert lib.ssr_scene_gather_tf(p, None, 0, 2, 64, 20, None, p, p, 1, 1, v, hip.F32, None) == -1       # no origins, W < 32
    assert lib.ssr_scene_gather_tf(p, None, 0, 4, 64, 20, p, p, p, 1, 3, v, hip.F32, None) == -1          # 9 channels, a pixel of 8, W < 32
    assert lib.ssr_scene_blend_add_tf(v, 7, p, p, 1, 3, p, p, 160, 200, p, None) == -2
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, p, 1, 3, p, p, 160, 202, p, None) == -2              # not 4 x a width
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, p, 1, 3, p, p, 124, 200, p, None) == -2              # lower than a chunk
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, None, 1, 3, p, p, 160, 200, p, None) == -1           # no transform ids
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, p, 1, 3, p, p, 160, 200, None, None) == -1           # no counter
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, p, 1, 3, p, p + 4, 160, 200, p, None) == -1          # accumulator not 16-byte aligned
    assert lib.ssr_scene_blend_add_tf(hip.View(p, 16, 0), hip.F32, p, p, 1, 9, p, p, 160, 200, p, None) == -1          # more than 8 channels
    assert lib.ssr_scene_blend_add_tf(hip.View(p, 8, 8), hip.F32, p, p, 1, 3, p, p, 160, 200, p, None) == -1           # channels outside the pixel
    assert lib.ssr_scene_blend_add_tf(v, 7, p, None, 1, 3, p, p, 160, 202, p, None) == -1                 # no transform ids, dtype, width
    assert lib.ssr_scene_blend_add_tf(v, 7, p, p, 1, 3, p, p, 160, 202, None, None) == -1                 # no counter, dtype, width
    assert lib.ssr_scene_blend_add_tf(v, hip.F32, p, p, 1, 3, p, p + 4, 124, 200, p, None) == -1          # accumulator alignment, height
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, 8 * 8191, p, 160, 202, None) == -2
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, 8 * 8191, p, 100, 200, None) == -2
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, 0, p, 160, 200, None) == -1                      # no scale
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, -5, p, 160, 200, None) == -1
    assert lib.ssr_scene_blend_finish_scaled(p, None, p, 3, 8 * 8191, p, 160, 200, None) == -1
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, 8 * 8191, p + 2, 160, 200, None) == -1           # mosaic not 4-byte aligned
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 9, 8 * 8191, p, 160, 200, None) == -1
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 3, 0, p, 160, 202, None) == -1                      # no scale, not 4 x a width
    assert lib.ssr_scene_blend_finish_scaled(p, None, p, 3, 8 * 8191, p, 160, 202, None) == -1            # no row sums, not 4 x a width
    assert lib.ssr_scene_blend_finish_scaled(p, p, p, 9, 8 * 8191, p, 100, 200, None) == -1               # 9 channels, lower than a chunk
    assert lib.ssr_abi_version() == 3
