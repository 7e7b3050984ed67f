"""GPU: which `ssr_scene_*` entry points a scene launches, in which order (satlas_super_resolution_amd/infer_scene.py).  The
docstrings promise that an absent option leaves the launches of the paths before it as they were; here `hip.lib` is replaced by a
recorder that forwards every call to the library, `super_resolve_scene` / `super_resolve_scene_blended` run with a tiny generator,
and the recorded names are held to the sequences written out below - they are the statement, nothing here is computed from the
code under test.  The generator runs between the gather side and the write-out side of every slice; only `ssr_scene_*` calls count.

    grid (every chunk on its own), 64 x 96: 6 chunks, batch 4 -> 2 slices; under the self-ensemble 48 rows -> 12 slices
    blended, 40 x 50 with overlap 8: 4 chunks, batch 3 -> 2 slices; under the self-ensemble 32 rows -> 11 slices"""
import functools
import random

import numpy as np
import pytest

from test_gpu_scene_bands import _small_model

pytestmark = pytest.mark.gpu

T, N = 3, 2                      # frames per scene, n_lr_images

# the frame choice
HEAD = {
    ("grid", "random"): ["zero_scan"],
    ("grid", "clearest"): ["frame_keys", "rank_frames"],
    ("blended", "random"): ["zero_scan_at"],
    ("blended", "clearest"): ["frame_keys", "rank_frames"],
    ("ensemble", "random"): ["zero_scan_at"],
    ("ensemble", "clearest"): ["frame_keys", "rank_frames"],
}
# one slice of chunks: (path, extra bands, nodata)
SLICE = {
    ("grid", 0, "fill"): ["gather", "scatter_u8"],
    ("grid", 0, "keep"): ["gather", "support_add", "scatter_u8"],
    ("grid", 1, "fill"): ["gather_bands", "scatter_u8"],
    ("grid", 1, "keep"): ["gather_bands", "support_add", "scatter_u8"],
    ("blended", 0, "fill"): ["gather_at", "blend_add"],
    ("blended", 0, "keep"): ["gather_at", "support_add", "blend_add"],
    ("blended", 1, "fill"): ["gather_bands", "blend_add"],
    ("blended", 1, "keep"): ["gather_bands", "support_add", "blend_add"],
}
# behind the last slice
TAIL = {
    ("grid", "fill"): [],
    ("grid", "keep"): ["apply_nodata"],
    ("blended", "fill"): ["blend_finish"],
    ("blended", "keep"): ["blend_finish", "apply_nodata"],
}
# the self-ensemble under `keep`: a slice of (chunk, transform) rows with and without some chunk's tf 0 row (rows 0, 8, 16, ...)
ENS_WITH = ["gather_tf", "support_add", "blend_add_tf"]
ENS_WITHOUT = ["gather_tf", "blend_add_tf"]
ENS_TAIL = ["blend_finish_scaled", "apply_nodata"]
# 48 rows in slices of 4: rows 0, 8, ... open every other slice; 32 rows in slices of 3: rows 0, 8, 16, 24 lie in slices 0, 2, 5, 8
ENS_SLICES = {"grid": "S.S.S.S.S.S.", "blended": "S.S..S..S.."}

SCENES = {"grid": (64, 96, None), "blended": (40, 50, 8)}
BATCH = {"grid": 4, "blended": 3}


class _Recorder:
    """the library with every `ssr_scene_*` look-up noted"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("ssr_scene_"):
            self.names.append(name[len("ssr_scene_"):])
        return fn


@functools.lru_cache(maxsize=None)
def _model(c_in):
    return _small_model(c_in)


def _scene(H, W, K):
    rng = np.random.RandomState(H + W)
    tci = rng.randint(1, 255, size=(T, H, W, 3)).astype(np.uint8)
    tci[0, :20, :20] = 0                            # some NODATA: frame 0 is a dirty frame of the first chunk
    bands = rng.randint(0, 256, size=(K, T, H, W)).astype(np.uint8) if K else None
    return tci, bands


def _launches(monkeypatch, path, K, frame_select, nodata, self_ensemble=False):
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene, super_resolve_scene_blended
    H, W, overlap = SCENES[path]
    tci, bands = _scene(H, W, K)
    model = _model(N * (3 + K))
    rec = _Recorder(hip.lib())
    monkeypatch.setattr(hip, "lib", lambda: rec)
    random.seed(5)
    kw = dict(batch=BATCH[path], bands=bands, frame_select=frame_select, nodata=nodata, self_ensemble=self_ensemble)
    if overlap is None:
        out = super_resolve_scene(model, tci, N, **kw)
    else:
        out = super_resolve_scene_blended(model, tci, N, overlap=overlap, **kw)
    assert out.shape == (4 * H, 4 * W, 3)
    return rec.names


@pytest.mark.parametrize("nodata", ["fill", "keep"])
@pytest.mark.parametrize("frame_select", ["random", "clearest"])
@pytest.mark.parametrize("K", [0, 1])
@pytest.mark.parametrize("path", ["grid", "blended"])
def test_the_launches_of_a_scene(monkeypatch, path, K, frame_select, nodata):
    expected = HEAD[path, frame_select] + 2 * SLICE[path, K, nodata] + TAIL[path, nodata]
    assert _launches(monkeypatch, path, K, frame_select, nodata) == expected


@pytest.mark.parametrize("frame_select", ["random", "clearest"])
@pytest.mark.parametrize("path", ["grid", "blended"])
def test_the_launches_of_a_self_ensembled_scene(monkeypatch, path, frame_select):
    expected = list(HEAD["ensemble", frame_select])
    for s in ENS_SLICES[path]:
        expected += ENS_WITH if s == "S" else ENS_WITHOUT
    expected += ENS_TAIL
    assert _launches(monkeypatch, path, 0, frame_select, "keep", self_ensemble=True) == expected
