"""CPU: the host half of the `frame_select: clearest` policy of scene inference (satlas_super_resolution_amd/infer_scene.py) - the
package's numpy statement of the rule, `rank_scene_frames`, against this file's own restatement (`window_counts`, `lexsort_rank`,
which tests/test_gpu_scene_select.py holds the kernels to), the property that the chosen set is one `select_scene_frames` can
return, the option's refusals and the declaration of the two device entry points.  Every comparison is exact integer equality."""
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT

ENTRIES = ("ssr_scene_frame_keys", "ssr_scene_rank_frames")


# ---------------------------------------------------------------- the rule, restated
def window_counts(tci, origins):
    """tci uint8 [T, H, W, 3], origins N x (y0, x0) -> (z, s), int64 [N, T]: per frame of the 32 x 32 window the pixels with at
    least one zero sample and the pixels whose three samples are all 255"""
    z = np.stack([(tci[:, y0:y0 + 32, x0:x0 + 32] == 0).any(axis=-1).sum(axis=(1, 2)) for y0, x0 in origins])
    s = np.stack([(tci[:, y0:y0 + 32, x0:x0 + 32] == 255).all(axis=-1).sum(axis=(1, 2)) for y0, x0 in origins])
    return z.astype(np.int64), s.astype(np.int64)


def keys_of(z, s):
    return (np.asarray(z, np.int64) << 16) | np.asarray(s, np.int64)


def lexsort_rank(key, n):
    """int32 [chunks, n]: per row the first n frames ordered by (key, frame index) ascending"""
    key = np.asarray(key)
    t = np.arange(key.shape[1])
    return np.stack([np.lexsort((t, k))[:n] for k in key]).astype(np.int32)


# ---------------------------------------------------------------- rank_scene_frames
@pytest.mark.parametrize("T", [1, 2, 5, 64, 65])
def test_rank_scene_frames_equals_the_lexsort_restatement(T):
    from satlas_super_resolution_amd.infer_scene import rank_scene_frames
    rng = np.random.RandomState(T)
    z = rng.choice([0, 0, 1, 7, 1024], size=(9, T))                      # a small value set: ties everywhere
    s = np.minimum(rng.choice([0, 3, 3, 500, 1024], size=(9, T)), 1024 - z)
    for n in sorted({1, min(8, T), T}):
        got = rank_scene_frames(z, s, n)
        assert got.dtype == np.int32 and got.shape == (9, n)
        assert np.array_equal(got, lexsort_rank(keys_of(z, s), n)), (T, n)
        assert all(len(set(row)) == n for row in got.tolist())
    with pytest.raises(ValueError):
        rank_scene_frames(z, s, T + 1)
    with pytest.raises(ValueError):
        rank_scene_frames(z, s, 0)


def test_lower_index_wins_ties_and_nodata_dominates_saturation():
    from satlas_super_resolution_amd.infer_scene import rank_scene_frames
    z = np.array([[0, 0, 0, 0], [1, 0, 0, 2], [0, 1, 0, 0], [3, 3, 3, 3]])
    s = np.array([[5, 5, 5, 5], [0, 1023, 1024, 0], [9, 0, 9, 8], [2, 1, 1, 0]])
    assert rank_scene_frames(z, s, 4).tolist() == [[0, 1, 2, 3],          # all equal: the frame order
                                                   [1, 2, 0, 3],          # a fully saturated clean frame before one NODATA pixel
                                                   [3, 0, 2, 1],          # fewest saturated first, the tie by index, NODATA last
                                                   [3, 1, 2, 0]]
    assert rank_scene_frames(z, s, 1).tolist() == [[0], [1], [3], [3]]    # the best frame comes first


@pytest.mark.parametrize("seed", range(4))
def test_the_chosen_set_is_one_the_reference_rule_can_draw_and_random_is_not_consumed(seed):
    from satlas_super_resolution_amd.infer_scene import rank_scene_frames, select_scene_frames
    rng = np.random.RandomState(seed)
    T, chunks = 7, 40
    has_zero = rng.rand(chunks, T) < rng.rand(chunks, 1)                 # rows from all clean to all dirty
    has_zero[0], has_zero[1] = False, True
    z = np.where(has_zero, rng.randint(1, 1025, size=(chunks, T)), 0)
    s = rng.randint(0, 1025, size=(chunks, T)) % (1025 - z)
    random.seed(seed)
    state = random.getstate()
    for n in (1, 3, 7):
        got = rank_scene_frames(z, s, n)
        for row, hz in zip(got.tolist(), has_zero):
            clean = set(np.flatnonzero(~hz).tolist())
            if len(clean) < n:                                           # every clean frame, topped up with dirty ones
                assert clean <= set(row) and len(set(row)) == n
                assert set(row[:len(clean)]) == clean                    # and the clean ones come first
            else:
                assert set(row) <= clean and len(set(row)) == n
    assert random.getstate() == state
    drawn = select_scene_frames(has_zero, 3)                             # what the reference's rule returns has the same shape of set
    for row, ref, hz in zip(rank_scene_frames(z, s, 3).tolist(), drawn.tolist(), has_zero):
        assert int(hz[row].sum()) == int(hz[ref].sum())                  # as many dirty frames as the rule is forced to take
    assert random.getstate() != state


# ---------------------------------------------------------------- the option and its refusals
def test_frame_select_values_are_checked_on_the_host():
    from satlas_super_resolution_amd.infer_scene import check_frame_select
    assert check_frame_select("random") == "random" and check_frame_select("clearest", 8, 8) == "clearest"
    assert check_frame_select("random", 5000, 9000) == "random"          # today's path keeps its own refusals
    for bad in ("best", "", None, "Clearest", 1):
        with pytest.raises(ValueError, match="frame_select"):
            check_frame_select(bad)
    with pytest.raises(ValueError, match="1024"):
        check_frame_select("clearest", 1025, 1)
    assert check_frame_select("clearest", 1024, 1024) == "clearest"
    with pytest.raises(ValueError, match="n_lr_images"):
        check_frame_select("clearest", 4, 5)


@pytest.mark.parametrize("blended", [False, True])
def test_scene_functions_refuse_before_touching_the_device(blended):
    import torch
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.infer_scene import scene_rank_frames, super_resolve_scene, super_resolve_scene_blended
    fn = super_resolve_scene_blended if blended else super_resolve_scene
    net = SSR_RRDBNet(num_in_ch=6, num_out_ch=3, num_feat=16, num_block=1, num_grow_ch=8)
    with pytest.raises(ValueError, match="frame_select"):
        fn(net, np.ones((3, 32, 64, 3), np.uint8), 2, frame_select="best")
    with pytest.raises(ValueError, match="n_lr_images"):                 # one frame of two: where random.sample raises today
        fn(net, np.ones((1, 32, 64, 3), np.uint8), 2, frame_select="clearest")
    with pytest.raises(ValueError, match="1024"):
        fn(net, np.ones((1025, 32, 32, 3), np.uint8), 2, frame_select="clearest")
    with pytest.raises(ValueError, match="1024"):
        scene_rank_frames(torch.zeros(1, 1025, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="n_lr_images"):
        scene_rank_frames(torch.zeros(1, 4, dtype=torch.int32), 5)


def test_driver_reads_frame_select(tmp_path):
    import torch
    from satlas_super_resolution_amd.infer_scene import run_infer_scene
    missing = str(tmp_path / "not_there") + "/"
    opt = {"data_dir": missing, "save_path": str(tmp_path / "out") + "/", "n_lr_images": 2, "io_workers": 1}
    with pytest.raises(ValueError, match="frame_select"):                # before the weights or the scene folder are looked at
        run_infer_scene(dict(opt, frame_select="cloudless"))
    with pytest.raises(ValueError, match="frame_select"):
        run_infer_scene(dict(opt, frame_select="cloudless", overlap=8, s2_bands=["tci", "b08"]))
    os.makedirs(tmp_path / "empty")
    opt["data_dir"] = str(tmp_path / "empty") + "/"
    for policy, want in (("clearest", "clearest"), ("random", "random"), (None, "random")):
        o = dict(opt) if policy is None else dict(opt, frame_select=policy)
        res = run_infer_scene(o, model=object(), device=torch.device("cpu"))             # no scenes: nothing reaches a device
        assert res["frame_select"] == want and (res["scenes"], res["chunks"]) == (0, 0)


# ---------------------------------------------------------------- interface
def test_select_entry_points_are_declared():
    from satlas_super_resolution_amd import hip
    src = open(os.path.join(ROOT, "include", "ssr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in hip.ABI_SYMBOLS


def test_select_entry_points_refuse_bad_arguments_without_a_launch():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    lib = hip.lib()
    p = 4096                                     # a non-null, aligned address: every call below returns before a launch
    assert lib.ssr_scene_frame_keys(p, 2, 31, 64, p, 1, p, None) == -2                       # smaller than a chunk
    assert lib.ssr_scene_frame_keys(p, 2, 64, 20, p, 1, p, None) == -2
    assert lib.ssr_scene_frame_keys(None, 2, 40, 50, p, 1, p, None) == -1
    assert lib.ssr_scene_frame_keys(p, 2, 40, 50, None, 1, p, None) == -1                    # no origins
    assert lib.ssr_scene_frame_keys(p, 2, 40, 50, p, 1, None, None) == -1                    # no keys
    assert lib.ssr_scene_frame_keys(p, 2, 40, 50, p, 1, p + 2, None) == -1                   # keys not 4-byte aligned
    assert lib.ssr_scene_frame_keys(p, 0, 40, 50, p, 1, p, None) == -1
    assert lib.ssr_scene_frame_keys(p, 2, 40, 50, p, 0, p, None) == -1
    assert lib.ssr_scene_frame_keys(p, 1 << 16, 40, 50, p, 1 << 15, p, None) == -1           # more than 2^30 items
    assert lib.ssr_scene_rank_frames(p, 1, 1025, 1, p, None) == -2                           # more than 1024 frames
    assert lib.ssr_scene_rank_frames(p, 1, 4, 5, p, None) == -2                              # n > T
    assert lib.ssr_scene_rank_frames(None, 1, 4, 2, p, None) == -1
    assert lib.ssr_scene_rank_frames(p, 1, 4, 2, None, None) == -1
    assert lib.ssr_scene_rank_frames(p, 0, 4, 2, p, None) == -1
    assert lib.ssr_scene_rank_frames(p, 1, 0, 1, p, None) == -1
    assert lib.ssr_scene_rank_frames(p, 1, 4, 0, p, None) == -1
    assert lib.ssr_scene_rank_frames(p + 1, 1, 4, 2, p, None) == -1
    assert lib.ssr_abi_version() == 3
