"""GPU: the `nodata: keep` policy of scene inference (satlas_super_resolution_amd/infer_scene.py; ssr_scene_support_add and
ssr_scene_apply_nodata of csrc/scene.hip) - the two kernels against the package's numpy statements of the policy (`scene_support`,
`apply_nodata`, which tests/test_scene_nodata_host.py holds to brute-force loops), `super_resolve_scene(_blended)(..., nodata="keep")`
on the grid, blended and bands paths against the `fill` result of the same call pushed through those statements with host-restated
frame ids, the untouched default, and the driver's option.  Every comparison is exact.  Fixture-sized generators only (num_feat 16,
num_block 1)."""
import os
import random

import numpy as np
import pytest
import torch

from test_gpu_scene_bands import _odd_base, _png, _pngs
from test_gpu_scene_select import _clearest_ids, _model, _random_ids
from test_scene_blend_host import grid_of
from test_scene_nodata_host import nodata_scene

pytestmark = pytest.mark.gpu

GUARD = 256
POISON = 77


def _guarded(shape, dtype, fill=0):
    """a device tensor of `shape` in the middle of a poisoned buffer: (the whole buffer, the view)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), POISON, dtype=dtype, device="cuda")
    view = big[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return big, view


def _guards_untouched(big):
    want = torch.tensor(POISON, dtype=big.dtype)
    return bool((big[:GUARD].cpu() == want).all()) and bool((big[-GUARD:].cpu() == want).all())


# ---------------------------------------------------------------- 1. the support kernel
def test_support_add_equals_the_numpy_restatement_at_any_origin_and_alignment():
    """3 W = 135 bytes per scene row: the rows of a window start at every byte offset of a word, whatever the base pointer.  Zeros
    per byte (about 5 %), one column zero in every frame, one whole frame zero; overlapping windows, two origins outside the scene
    and a chunk with a frame id of T, which add nothing."""
    from satlas_super_resolution_amd.infer_scene import scene_support, scene_support_add
    T, H, W, n = 5, 70, 45, 3
    tci = nodata_scene(11, T, H, W)
    rng = np.random.RandomState(12)
    origins = [(0, 0), (38, 13), (37, 12), (H - 32, W - 32), (39, 0), (0, 14), (3, 3)]       # (39, 0), (0, 14): outside the scene
    ids = np.stack([rng.permutation(T)[:n] for _ in origins]).astype(np.int32)
    ids[0] = (3, 0, 1)                             # the frame that is zero everywhere fills a slot
    ids[2] = (4, 4, 2)                             # a frame in two slots counts twice
    ids[-1] = (0, T, 1)                            # a frame id outside the scene: the gathers skip this chunk, so does the count
    want = scene_support(tci, origins, ids)
    assert (want[:, 17] == 0).all() and want.max() > n and (want > 0).sum() > 1500
    assert np.array_equal(want, scene_support(tci, origins[:4], ids[:4]))
    org = torch.tensor(origins, dtype=torch.int32, device="cuda")
    fid = torch.from_numpy(ids).cuda()
    for name, dev in (("aligned", torch.from_numpy(tci).cuda()), ("odd base", _odd_base(tci))):
        big, support = _guarded((H, W), torch.int32)
        scene_support_add(dev, org, fid, support)
        torch.cuda.synchronize()
        got = support.cpu().numpy()
        print(f"[{name}] differing words {int((got != want).sum())} of {want.size}")
        assert np.array_equal(got, want), name
        scene_support_add(dev, org, fid, support)  # it ADDS to what support holds
        torch.cuda.synchronize()
        assert np.array_equal(support.cpu().numpy(), 2 * want), name
        assert _guards_untouched(big), name


# ---------------------------------------------------------------- 2. the apply kernel
@pytest.mark.parametrize("C", [1, 3, 4])
def test_apply_nodata_equals_the_numpy_restatement(C):
    """a 132 x 140 mosaic: with C = 3 the aligned 4-byte units straddle output pixels and, every fourth pixel, low-resolution pixels"""
    from satlas_super_resolution_amd.infer_scene import apply_nodata, scene_apply_nodata, support_to_u8
    rng = np.random.RandomState(20 + C)
    H, W = 33, 35
    support = rng.randint(0, 4, size=(H, W)).astype(np.int32)
    support[5, 7:11] = (254, 255, 256, 70000)
    mosaic = rng.randint(0, 256, size=(4 * H, 4 * W, C)).astype(np.uint8)
    mosaic[rng.rand(4 * H, 4 * W, C) < 0.1] = 0    # zeros inside supported pixels: they become 1
    sup = torch.from_numpy(support).cuda()
    for m in (1, 2):
        want = apply_nodata(mosaic, support, m)
        up = np.repeat(np.repeat(support, 4, 0), 4, 1)
        assert ((mosaic == 0) & (up >= m)[:, :, None]).sum() > 100 and (up < m).sum() > 1000
        for with_u8 in (False, True):
            big, dev = _guarded(mosaic.shape, torch.uint8)
            dev.copy_(torch.from_numpy(mosaic))
            big8, u8 = _guarded((H, W), torch.uint8, fill=99)
            scene_apply_nodata(dev, sup, m, u8 if with_u8 else None)
            torch.cuda.synchronize()
            got = dev.cpu().numpy()
            print(f"[C {C}, min_support {m}, support_u8 {with_u8}] differing bytes {int((got != want).sum())} of {want.size}")
            assert np.array_equal(got, want), (C, m, with_u8)
            assert _guards_untouched(big) and _guards_untouched(big8), (C, m, with_u8)
            if with_u8:
                assert np.array_equal(u8.cpu().numpy(), support_to_u8(support)), (C, m)
                assert u8.cpu().numpy()[5, 7:11].tolist() == [254, 255, 255, 255]
            else:
                assert (u8.cpu().numpy() == 99).all(), (C, m)             # a null support_u8: nothing is written anywhere
    assert np.array_equal(sup.cpu().numpy(), support)                    # the support map is read only


# ---------------------------------------------------------------- 3. end to end
BLOCK = (slice(44, 60), slice(24, 44))             # 16 x 20 = 320 pixels, zero in three of the five frames


def _scene(seed, T, H, W):
    """no zero but what is planted: the wedge x + y < 40 in EVERY frame, BLOCK in frames 0 .. 2, column 40 of frame 1"""
    assert T == 5
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    tci = np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 254).astype(np.uint8)
    tci[:, yy + xx < 40] = 0
    tci[(slice(0, 3),) + BLOCK] = 0
    tci[1, :, 40] = 0
    return tci, yy + xx < 40


def _up(a):
    return np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)


def _keep_checks(call, tci, wedge, origins, n, policy):
    """what every path is held to, for min_support 1 (the wedge is masked) and n (the block, where only two frames have data, too)"""
    from satlas_super_resolution_amd.infer_scene import apply_nodata, scene_support, support_to_u8
    H, W = tci.shape[1:3]
    seed = 5

    def run(**kw):
        random.seed(seed)
        return call(frame_select=policy, **kw)

    ids = _clearest_ids(tci, origins, n) if policy == "clearest" else _random_ids(tci, origins, n, seed)
    support = scene_support(tci, origins, ids)
    assert wedge.sum() == 820 and (support[wedge] == 0).all() and (support[~wedge] > 0).mean() > 0.9
    fill = run().copy()
    assert fill.dtype == np.uint8 and fill.shape == (4 * H, 4 * W, 3)
    assert fill[_up(wedge)].any()                  # under `fill` the generator's invention stands in the wedge
    shares = []
    for m in (1, n):
        masked = support < m
        share = masked.sum() / masked.size
        print(f"[{policy}, min_support {m}] masked low-resolution pixels {int(masked.sum())} of {masked.size} ({100 * share:.1f} %), "
              f"largest support {int(support.max())}")
        assert 0.05 < share < 0.50                 # neither an all-masked nor a never-masked scene
        shares.append(int(masked.sum()))
        want = apply_nodata(fill, support, m)
        got, sup8 = run(nodata="keep", min_support=m, return_support=True)
        got, sup8 = got.copy(), sup8.copy()
        print(f"[{policy}, min_support {m}] differing bytes {int((got != want).sum())} of {want.size}")
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert not np.array_equal(got, fill)
        assert not got[_up(wedge)].any()           # the wedge is all zeros
        assert (got[_up(~masked)] >= 1).all()      # outside masked pixels no sample is 0
        assert sup8.dtype == np.uint8 and sup8.shape == (H, W) and np.array_equal(sup8, support_to_u8(support))
        again, sup8b = run(nodata="keep", min_support=m, return_support=True)
        assert np.array_equal(again, got) and np.array_equal(sup8b, sup8)                    # two runs: identical bytes
        assert np.array_equal(run(nodata="keep", min_support=m), got)                        # without return_support: the mosaic alone
    assert shares[1] > shares[0]                   # the block, 2 frames with data of n = 3 slots, is masked by min_support = n only
    return support


@pytest.mark.parametrize("policy", ["random", "clearest"])
def test_grid_path_keeps_nodata(policy):
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene
    T, H, W, n = 5, 64, 96, 3
    tci, wedge = _scene(51, T, H, W)
    model = _model(3 * n)
    support = _keep_checks(lambda **kw: super_resolve_scene(model, tci, n, batch=4, **kw), tci, wedge, grid_of(H, W, 0), n, policy)
    assert support.max() == n                      # one covering chunk per pixel
    if policy == "clearest":                       # a device tensor, one batch
        random.seed(5)
        got, sup8 = super_resolve_scene(model, torch.from_numpy(tci).cuda(), n, frame_select=policy, nodata="keep", return_support=True)
        assert np.array_equal(sup8, np.minimum(support, 255)) and not got[_up(wedge)].any()


@pytest.mark.parametrize("policy", ["random", "clearest"])
def test_blended_path_keeps_nodata(policy):
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene_blended
    T, H, W, n, overlap = 5, 70, 45, 3, 8
    tci, wedge = _scene(52, T, H, W)
    origins = grid_of(H, W, overlap)
    assert origins == [(0, 0), (0, 13), (24, 0), (24, 13), (38, 0), (38, 13)]
    model = _model(3 * n)
    support = _keep_checks(lambda **kw: super_resolve_scene_blended(model, tci, n, overlap=overlap, batch=4, **kw), tci, wedge,
                           origins, n, policy)
    assert support.max() == 4 * n                  # two chunks per axis cover the middle


def test_bands_path_keeps_nodata():
    """K = 1 and the 4 n-channel generator; zeros in the band take no part in the support"""
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene
    T, H, W, n, K = 5, 64, 96, 3, 1
    tci, wedge = _scene(53, T, H, W)
    rng = np.random.RandomState(54)
    bands = rng.randint(1, 256, size=(K, T, H, W)).astype(np.uint8)
    bands[0, :, 50:64, 60:96] = 0                  # NODATA in the band alone: the pixels keep their support
    model = _model(n * (3 + K))
    support = _keep_checks(lambda **kw: super_resolve_scene(model, tci, n, batch=4, bands=bands, **kw), tci, wedge, grid_of(H, W, 0),
                           n, "clearest")
    assert (support[50:64, 60:96] == n).all()


def test_a_nan_under_a_masked_pixel_still_raises():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene, super_resolve_scene_blended
    n = 3
    model = _model(3 * n)
    frames = np.zeros((5, 32, 64, 3), np.uint8)    # all NODATA: every pixel is masked
    for fn in (super_resolve_scene, super_resolve_scene_blended):
        got, sup8 = fn(model, frames, n, frame_select="clearest", nodata="keep", return_support=True)
        assert not got.any() and not sup8.any()

    class Poisoned:
        """the generator with a NaN written into the plan's output behind every forward"""
        kwargs, compute_dtype = model.kwargs, model.compute_dtype

        def parameters(self):
            return model.parameters()

        def plan_for_inference(self, *a):
            return model.plan_for_inference(*a)

        def run_forward(self, p):
            model.run_forward(p)
            p.out.view(-1)[0] = float("nan")

    for fn in (super_resolve_scene, super_resolve_scene_blended):
        with pytest.raises(FloatingPointError):
            fn(Poisoned(), frames, n, frame_select="clearest", nodata="keep")


# ---------------------------------------------------------------- 4. the default is untouched
def test_fill_is_the_call_without_the_argument():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene, super_resolve_scene_blended
    n = 3
    model = _model(3 * n)
    for fn, (H, W), kw in ((super_resolve_scene, (64, 96), {}), (super_resolve_scene_blended, (70, 45), {"overlap": 8})):
        tci, wedge = _scene(55, 5, H, W)
        random.seed(6)
        today = fn(model, tci, n, batch=4, **kw).copy()
        random.seed(6)
        got = fn(model, tci, n, batch=4, nodata="fill", **kw)
        assert isinstance(got, np.ndarray) and np.array_equal(got, today)
        random.seed(6)
        assert np.array_equal(fn(model, tci, n, batch=4, nodata="fill", min_support=1, return_support=False, **kw), today)
        assert today[_up(wedge)].any()


# ---------------------------------------------------------------- 5. the driver's `nodata:` option
def test_driver_with_nodata_keep_writes_the_support_map(tmp_path):
    from PIL import Image
    from satlas_super_resolution_amd.infer_scene import run_infer_scene, super_resolve_scene
    T, H, W, n = 5, 64, 96, 3
    tci, wedge = _scene(56, T, H, W)
    os.makedirs(tmp_path / "scenes")
    Image.fromarray(tci.reshape(T * H, W, 3)).save(tmp_path / "scenes" / "a.png")
    model = _model(3 * n)
    opt = {"data_dir": str(tmp_path / "scenes") + "/", "save_path": str(tmp_path / "out") + "/", "n_lr_images": n, "scene_hw": [H, W],
           "io_workers": 2, "nodata": "keep", "nodata_min_support": n}
    random.seed(9)
    res = run_infer_scene(opt, model=model)
    assert (res["scenes"], res["chunks"], res["nodata"], res["nodata_min_support"]) == (1, 6, "keep", n)
    assert _pngs(str(tmp_path / "out")) == ["a/stitched_s2.png", "a/stitched_sr.png", "a/stitched_support.png"]
    random.seed(9)
    want, sup8 = super_resolve_scene(model, tci, n, nodata="keep", min_support=n, return_support=True)
    assert np.array_equal(_png(tmp_path / "out" / "a" / "stitched_sr.png"), want)
    assert np.array_equal(_png(tmp_path / "out" / "a" / "stitched_s2.png"), tci[0])         # stays frame 0
    gray = _png(tmp_path / "out" / "a" / "stitched_support.png")
    assert gray.dtype == np.uint8 and gray.shape == (H, W) and np.array_equal(gray, sup8)
    assert not want[_up(wedge)].any() and sup8.max() == n
    # without the key: the two files and the dictionary of today
    plain = {k: v for k, v in opt.items() if not k.startswith("nodata")}
    plain["save_path"] = str(tmp_path / "out2") + "/"
    random.seed(9)
    res = run_infer_scene(plain, model=model)
    assert sorted(res) == ["chunks", "frame_select", "io_workers", "scenes", "seconds"]
    assert _pngs(str(tmp_path / "out2")) == ["a/stitched_s2.png", "a/stitched_sr.png"]
    assert not os.path.exists(tmp_path / "out2" / "a" / "stitched_support.png")
    random.seed(9)
    assert np.array_equal(_png(tmp_path / "out2" / "a" / "stitched_sr.png"), super_resolve_scene(model, tci, n))
