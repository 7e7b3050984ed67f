"""GPU: the self-ensemble of scene inference (satlas_super_resolution_amd/infer_scene.py `self_ensemble`; ssr_scene_gather_tf,
ssr_scene_blend_add_tf and ssr_scene_blend_finish_scaled of csrc/scene.hip) - the gather against `ensemble_transform` of the existing
layout and against the existing gathers, the blend-add and the finish against `ensemble_accumulate` / `ensemble_finish` of
tests/test_scene_ensemble_host.py, `super_resolve_scene_blended(..., self_ensemble=True)` against the module's forward through that
restatement, the exact symmetry the option gives scene inference, the other options beside it, the untouched defaults and the driver's
key.  Every comparison is exact.  Fixture-sized generators only (num_feat 16, num_block 1)."""
import functools
import os
import random

import numpy as np
import pytest
import torch

from test_scene_blend_host import grid_of
from test_scene_ensemble_host import ensemble_accumulate, ensemble_finish, ensemble_rows

pytestmark = pytest.mark.gpu


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path)).copy()


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f.endswith(".png"))


def _layout(tci, bands, origin, ids):
    """a chunk as the existing gathers lay it out, uint8 [32, 32, n (3 + K)]: per chosen frame the TCI, then the bands"""
    (y0, x0), parts = origin, []
    for f in ids:
        parts.append(tci[f, y0:y0 + 32, x0:x0 + 32])
        if bands is not None:
            parts.append(bands[:, f, y0:y0 + 32, x0:x0 + 32].transpose(1, 2, 0))
    return np.concatenate(parts, axis=-1)


def _odd_base(a, off):
    """the array on the device, `off` bytes into a buffer: an odd base address"""
    big = torch.zeros(a.size + off, dtype=torch.uint8, device="cuda")
    big[off:] = torch.from_numpy(a).cuda().reshape(-1)
    return big[off:].view(a.shape)


# ---------------------------------------------------------------- 1. the gather
H1, W1 = 45, 51                                    # a row of the scene is 153 bytes: rows and windows start at every alignment


# T = 3 with n = 1 and 3, K = 0 and 2: 3, 9, 5 and 15 channels, element stores; T = 4, n = 4 with K = 0 (12 channels: the 16-byte
# fp32 stores) and K = 1 (16 channels: the 16-byte stores of both storage types)
@pytest.mark.parametrize("storage,T,n,K", [(s, 3, n, K) for s in ("fp32", "bf16") for n in (1, 3) for K in (0, 2)]
                         + [("fp32", 4, 4, 0), ("fp32", 4, 4, 1), ("bf16", 4, 4, 1)])
def test_gather_tf_equals_the_transform_of_the_existing_layout_bit_for_bit(storage, T, n, K):
    from satlas_super_resolution_amd import hip
    from satlas_super_resolution_amd.infer_scene import ensemble_transform, scene_gather_at, scene_gather_bands, scene_gather_tf
    rng = np.random.RandomState(100 * n + K)
    tci = rng.randint(0, 256, size=(T, H1, W1, 3)).astype(np.uint8)
    bands = rng.randint(0, 256, size=(K, T, H1, W1)).astype(np.uint8) if K else None
    assert len(np.unique(tci)) == 256                                    # every byte value goes through the conversion
    places = [(5, 7), (H1 - 32, W1 - 32)]                                # odd origins; the last legal origin
    origins = [o for o in places for _ in range(8)] + [(5, 7), (H1 - 31, 7)]
    tfs = [tf for _ in places for tf in range(8)] + [9, 3]               # the last two rows: a bad transform id, an origin outside
    B, C = len(origins), n * (3 + K)
    cs = -(-C // 8) * 8
    ids = np.stack([rng.permutation(T)[:n] for _ in range(B)]).astype(np.int32)
    dt = hip.dtype_code(storage)
    tdt = hip.torch_dtype(dt)
    inv255 = torch.tensor(np.float32(1.0) / np.float32(255.0))
    want = torch.full((B, 32, 32, cs), -7.0, dtype=tdt)
    for b in range(16):
        chunk = np.ascontiguousarray(ensemble_transform(_layout(tci, bands, origins[b], ids[b]), tfs[b]))
        want[b, :, :, :C] = (torch.from_numpy(chunk).float() * inv255).to(tdt)       # x * (1 / 255) in fp32, then the cast
    d_tci = _odd_base(tci, 3)
    d_bands = _odd_base(bands, 1) if K else None
    d_org = torch.tensor(origins, dtype=torch.int32, device="cuda")
    d_ids = torch.from_numpy(ids).cuda()
    got = torch.full((B, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    scene_gather_tf(d_tci, d_bands, d_org, d_ids, torch.tensor(tfs, dtype=torch.int32, device="cuda"), got, dt)
    torch.cuda.synchronize()
    bits = torch.int32 if storage == "fp32" else torch.int16
    diff = int((got.cpu().view(bits) != want.view(bits)).sum())
    print(f"[{storage}, T = {T}, n = {n}, K = {K}] differing elements {diff} of {want.numel()}")
    assert diff == 0
    assert bool((got[16:] == -7.0).all()) and bool((got[..., C:] == -7.0).all())     # the two skipped rows, the pad channels
    assert float(got[:16, ..., :C].float().min()) >= 0.0
    # the tf = 0 rows against the existing kernels
    zero = [0, 8]
    old = torch.full((2, 32, 32, cs), -7.0, dtype=tdt, device="cuda")
    if K:
        scene_gather_bands(d_tci, d_bands, d_org[zero].contiguous(), d_ids[zero].contiguous(), old, dt)
    else:
        scene_gather_at(d_tci, d_org[zero].contiguous(), d_ids[zero].contiguous(), old, dt)
    torch.cuda.synchronize()
    assert torch.equal(got[zero].view(bits), old.view(bits))


# ---------------------------------------------------------------- 2. blend-add and finish against the numpy restatement
def _synthetic_outputs(N, C, cs, seed):
    """[N, 128, 128, cs] fp32: values below 0 and above 1, exactly 0 and 1, multiples of 1/255 and their neighbours, a NaN, a +Inf and
    a -Inf among the C output channels (3 non-finite samples) and a NaN in a pad channel, which is no output sample"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.rand(N, 128, 128, cs, generator=g) * 1.6 - 0.3
    k = torch.randint(0, 256, (N, 128, 16, cs), generator=g).float() / 255
    buf[:, :, :16] = k
    buf[:, :, 16:32] = torch.where(torch.rand(k.shape, generator=g) < 0.5, torch.nextafter(k, torch.tensor(2.0)), torch.nextafter(k, torch.tensor(-1.0)))
    buf[:, 7, 40:50] = 0.0
    buf[:, 9, 40:50] = 1.0
    buf[0, 100, 100, 1] = float("nan")
    buf[N - 1, 127, 127, C - 1] = float("inf")
    buf[N // 2, 0, 0, 0] = float("-inf")
    buf[1, 64, 3, C] = float("nan")
    return buf, 3


def _ensemble_on_device(src, origins, tfs, order, splits, C, H, W, overlap, dt):
    """the rows in `order`, cut into launches at `splits` -> (accumulator uint32 [4H, 4W, C], counter, mosaic) as numpy"""
    from satlas_super_resolution_amd.infer_scene import (ENSEMBLE, ENSEMBLE_ONE, blend_weight_sums, blend_window, scene_blend_add_tf,
                                                         scene_blend_finish_scaled)
    acc = torch.zeros(4 * H, 4 * W, C, dtype=torch.int32, device="cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    window = torch.from_numpy(blend_window(overlap)).cuda()
    org = torch.tensor([origins[i] for i in order], dtype=torch.int32, device="cuda")
    tf = torch.tensor([tfs[i] for i in order], dtype=torch.int32, device="cuda")
    s = src[list(order)].contiguous()
    bounds = [0] + list(splits) + [len(order)]
    for a, b in zip(bounds[:-1], bounds[1:]):
        scene_blend_add_tf(s[a:b], org[a:b].contiguous(), tf[a:b].contiguous(), C, window, acc, counter, dt)
    mosaic = torch.full((4 * H, 4 * W, C), 9, dtype=torch.uint8, device="cuda")
    scene_blend_finish_scaled(acc, torch.from_numpy(blend_weight_sums(H, overlap)).cuda(),
                              torch.from_numpy(blend_weight_sums(W, overlap)).cuda(), mosaic, ENSEMBLE * ENSEMBLE_ONE)
    torch.cuda.synchronize()
    return acc.cpu().numpy().view(np.uint32), int(counter[0]), mosaic.cpu().numpy()


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("H,W,overlap", [(49, 50, 16), (40, 56, 8)])
def test_blend_add_tf_and_finish_equal_the_numpy_restatement_in_any_order_and_grouping(storage, H, W, overlap):
    from satlas_super_resolution_amd import hip
    C, cs = 3, 8
    chunks = grid_of(H, W, overlap)
    assert len(chunks) == {(49, 50): 9, (40, 56): 4}[(H, W)]
    origins, tfs = ensemble_rows(chunks)
    N = len(origins)
    origins = origins + [(H - 31, 0), (0, 0)]                            # two rows that add nothing and count nothing: an origin
    tfs = tfs + [2, -1]                                                  # outside the scene, a transform id outside 0 .. 7
    buf, planted = _synthetic_outputs(N + 2, C, cs, seed=H)
    buf[N, 5, 5, 0] = buf[N + 1, 6, 6, 1] = float("nan")                 # (in the skipped rows)
    buf[N + 1, 127, 127, C - 1] = 0.5                                    # (_synthetic_outputs put its +Inf into a skipped row)
    buf[N - 1, 127, 127, C - 1] = float("inf")
    dt = hip.dtype_code(storage)
    src = buf.to(hip.torch_dtype(dt)).cuda().contiguous()
    outs = src[..., :C].float().cpu().numpy()                            # the stored values, widened exactly
    want_acc = ensemble_accumulate(outs, origins, tfs, H, W, overlap)
    want = ensemble_finish(want_acc, H, W, overlap)
    fwd = list(range(N))
    runs = [("one launch", fwd, []), ("reversed", fwd[::-1], []), ("two launches", fwd, [13]),      # 13: inside the second chunk
            ("with the skipped rows", [N, N + 1] + fwd, [])]
    for name, order, splits in runs:
        acc, bad, mosaic = _ensemble_on_device(src, origins, tfs, order, splits, C, H, W, overlap, dt)
        print(f"[{storage} {H} x {W} overlap {overlap}, {name}] differing accumulator words {int((acc != want_acc).sum())}, "
              f"differing bytes {int((mosaic != want).sum())} of {want.size}, counter {bad}")
        assert bad == planted
        assert np.array_equal(acc, want_acc)
        assert np.array_equal(mosaic, want)
    assert len(np.unique(want)) > 200


def test_the_largest_accumulator_value_every_sample_one_under_nine_fold_cover_of_eight_rows():
    from satlas_super_resolution_amd import hip
    H, W, overlap, C = 49, 50, 16, 3
    origins, tfs = ensemble_rows(grid_of(H, W, overlap))
    src = torch.ones(72, 128, 128, 8, device="cuda")
    want_acc = ensemble_accumulate(np.ones((72, 128, 128, C), np.float32), origins, tfs, H, W, overlap)
    acc, bad, mosaic = _ensemble_on_device(src, origins, tfs, range(72), [], C, H, W, overlap, hip.dtype_code("fp32"))
    print(f"largest accumulator word {int(want_acc.max())} = {int(want_acc.max()) / 2 ** 32:.3f} x 2^32")
    assert int(want_acc.max()) > 2 ** 29 and bad == 0
    assert int(acc.max()) == int(want_acc.max()) and np.array_equal(acc, want_acc)
    assert (mosaic == 255).all()


# ---------------------------------------------------------------- 3. end to end against the module
@functools.lru_cache(maxsize=None)
def _small_model(c_in, compute_dtype="fp32h"):
    from oracle import esrgan_oracle as O
    from oracle import make_infer_golden as M
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    sd = O.generator_init(num_in_ch=c_in, num_out_ch=3, scale=4, seed=M.SEED, **M.G_KW)
    sd["conv_last.bias"] = torch.full_like(sd["conv_last.bias"], 0.45)
    sd["conv_last.weight"] = sd["conv_last.weight"] * 8
    net = SSR_RRDBNet(num_in_ch=c_in, num_out_ch=3, compute_dtype=compute_dtype, **M.G_KW)
    net.load_state_dict(sd, strict=True)
    return net.cuda().eval().freeze_packed()


def _smooth_scene(seed, T, H, W):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 120 + 70 * np.sin(yy / 9.0)[None, :, :, None] * np.cos(xx / 13.0)[None, :, :, None]
    return np.clip(base + rng.randint(-25, 26, size=(T, H, W, 3)), 1, 254).astype(np.uint8)


def test_self_ensembled_scene_is_the_modules_rows_through_the_numpy_restatement():
    from satlas_super_resolution_amd.infer_scene import ensemble_transform, super_resolve_scene_blended
    from satlas_super_resolution_amd.utils.infer_utils import frames_to_input, select_frames
    T, H, W, n, batch, overlap = 4, 40, 56, 2, 8, 8
    scene = _smooth_scene(22, T, H, W)
    chunks = grid_of(H, W, overlap)
    assert chunks == [(0, 0), (0, 24), (8, 0), (8, 24)]
    scene[0, 3, 5, 1] = 0                          # in the chunk at (0, 0) only: one zero-holding frame
    scene[1, 39, 54, 0] = scene[2, 38, 55, 2] = scene[3, 39, 55, 2] = 0          # chunk (8, 24) only: one clean frame, topped up
    model = _small_model(3 * n)
    random.seed(5)
    got = super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch, self_ensemble=True)
    assert got.dtype == np.uint8 and got.shape == (4 * H, 4 * W, 3)
    got = got.copy()
    # select_frames chunk by chunk in row-major order, once per chunk; the rows chunk-major with tf 0 .. 7, the same batch grouping
    random.seed(5)
    sels = [select_frames(scene[:, y0:y0 + 32, x0:x0 + 32].reshape(T * 32, 32, 3), n)[0] for y0, x0 in chunks]
    rows = []
    for sel in sels:                               # [n, 32, 32, 3]: the transform acts on the two spatial axes of every frame
        assert sel.shape == (n, 32, 32, 3)
        for tf in range(8):
            rows.append(np.ascontiguousarray(ensemble_transform(sel.transpose(1, 2, 0, 3), tf).transpose(2, 0, 1, 3)))
    outs = []
    with torch.no_grad():
        for r0 in range(0, len(rows), batch):
            x = frames_to_input(torch.from_numpy(np.stack(rows[r0:r0 + batch])).cuda())
            outs.append(model(x).float().permute(0, 2, 3, 1).cpu().numpy())
    origins, tfs = ensemble_rows(chunks)
    want = ensemble_finish(ensemble_accumulate(np.concatenate(outs), origins, tfs, H, W, overlap), H, W, overlap)
    print(f"differing bytes {int((got != want).sum())} of {want.size}")
    assert np.array_equal(got, want)
    assert float(got.std()) > 5
    random.seed(5)
    assert np.array_equal(super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch, self_ensemble=True), got)
    random.seed(5)
    assert np.array_equal(super_resolve_scene_blended(model, torch.from_numpy(scene).cuda(), n, overlap=overlap, batch=batch,
                                                      self_ensemble=True), got)
    random.seed(5)                                 # integer sums: rows cut at 5, inside the chunks, add the same words
    assert np.array_equal(super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=5, self_ensemble=True), got)
    random.seed(5)                                 # `random` is consumed once per chunk, as without the option
    super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch)
    plain_state = random.getstate()
    random.seed(5)
    super_resolve_scene_blended(model, scene, n, overlap=overlap, batch=batch, self_ensemble=True)
    assert random.getstate() == plain_state


# ---------------------------------------------------------------- 4. the symmetry
def _turn_scene(scene, g):
    """[T, H, W, 3] under the symmetry g of its two spatial axes"""
    from satlas_super_resolution_amd.infer_scene import ensemble_transform
    return np.ascontiguousarray(ensemble_transform(scene.transpose(1, 2, 0, 3), g).transpose(2, 0, 1, 3))


def test_the_self_ensembled_mosaic_of_a_turned_scene_is_the_turned_mosaic():
    """the test that cannot pass without the option: an exact symmetry of scene inference.  The chunk origins of a 40 x 56 scene
    with overlap 8 are [0, 8] x [0, 24], symmetric about the centre, `clearest` keys do not change when a chunk is flipped or
    transposed, and every frame has its own number of planted zeros in every chunk, so no choice is a tie on the frame index."""
    from satlas_super_resolution_amd.infer_scene import (ensemble_transform, rank_scene_frames, scene_chunk_origins,
                                                         super_resolve_scene_blended)
    T, H, W, n, overlap = 4, 40, 56, 2, 8
    ys, xs = scene_chunk_origins(H, overlap), scene_chunk_origins(W, overlap)
    assert ys == [0, 8] and xs == [0, 24]
    assert [H - 32 - y for y in reversed(ys)] == ys and [W - 32 - x for x in reversed(xs)] == xs      # symmetric about the centre
    scene = _smooth_scene(31, T, H, W)
    # zeros in the corner that one chunk alone covers (8 x 24 pixels): frame t gets counts[chunk][t] of them
    counts = {(0, 0): [0, 1, 2, 3], (0, 24): [3, 0, 1, 2], (8, 0): [2, 3, 0, 1], (8, 24): [1, 2, 3, 0]}
    for (y0, x0), per_frame in counts.items():
        cy, cx = (2 if y0 == 0 else 37), (3 if x0 == 0 else 50)
        for t, k in enumerate(per_frame):
            scene[t, cy, cx:cx + k, t % 3] = 0
    z = np.array([[(scene[t, y0:y0 + 32, x0:x0 + 32] == 0).any(axis=-1).sum() for t in range(T)] for (y0, x0) in counts])
    assert z.tolist() == list(counts.values())
    assert rank_scene_frames(z, np.zeros_like(z), n).tolist() == [[0, 1], [1, 2], [2, 3], [3, 0]]   # the choice differs by chunk
    model = _small_model(3 * n)
    kw = dict(overlap=overlap, batch=8, frame_select="clearest")
    mosaic = super_resolve_scene_blended(model, scene, n, self_ensemble=True, **kw).copy()
    plain = super_resolve_scene_blended(model, scene, n, **kw).copy()
    assert float(mosaic.std()) > 5 and not np.array_equal(mosaic, plain)
    plain_breaks = []
    for g in range(8):
        turned = _turn_scene(scene, g)
        assert turned.shape == ((T, W, H, 3) if g & 4 else (T, H, W, 3))
        got = super_resolve_scene_blended(model, turned, n, self_ensemble=True, **kw)
        want = ensemble_transform(mosaic, g)
        print(f"[g = {g}] self-ensemble: differing bytes {int((got != want).sum())} of {want.size}")
        assert np.array_equal(got, want), g
        other = super_resolve_scene_blended(model, turned, n, **kw)
        plain_breaks.append(int((other != ensemble_transform(plain, g)).sum()))
    print(f"the plain blended path, differing bytes per symmetry: {plain_breaks}")
    assert plain_breaks[0] == 0 and max(plain_breaks) > 0                 # the plain path is not symmetric: the test can tell


# ---------------------------------------------------------------- 5. with the other options
def _up(a):
    return np.repeat(np.repeat(a, 4, axis=0), 4, axis=1)


def test_self_ensemble_with_bands_and_nodata_keep():
    from satlas_super_resolution_amd.infer_scene import apply_nodata, super_resolve_scene, super_resolve_scene_blended
    T, H, W, n, K, overlap = 4, 40, 56, 2, 1, 8
    tci = _smooth_scene(41, T, H, W)
    yy, xx = np.mgrid[0:H, 0:W]
    corner = yy + xx < 20
    tci[:, corner] = 0                             # a NODATA corner in every frame
    tci[:3, 30:36, 40:50] = 0                      # and a block with data in one frame only
    bands = np.random.RandomState(42).randint(1, 256, size=(K, T, H, W)).astype(np.uint8)
    model = _small_model(n * (3 + K))
    kw = dict(overlap=overlap, batch=8, bands=bands, frame_select="clearest")
    _, support = super_resolve_scene_blended(model, tci, n, nodata="keep", return_support=True, **kw)
    support = support.copy()
    fill = super_resolve_scene_blended(model, tci, n, self_ensemble=True, **kw).copy()
    assert not np.array_equal(fill, super_resolve_scene_blended(model, tci, n, **kw))
    for m in (1, 3):
        got, sup = super_resolve_scene_blended(model, tci, n, nodata="keep", min_support=m, return_support=True, self_ensemble=True, **kw)
        assert np.array_equal(sup, support)        # the support map is what it is without the option: once per chunk
        masked = _up(support < m)
        assert 0.02 < masked.mean() < 0.5
        assert not got[masked].any() and (got[~masked] >= 1).all()
        assert np.array_equal(got, apply_nodata(fill, support, m))
    assert (support[corner] == 0).all() and support.max() == 4 * n
    # a batch that cuts the rows inside the chunks: support is still added once per chunk
    got5, sup5 = super_resolve_scene_blended(model, tci, n, nodata="keep", min_support=3, return_support=True, self_ensemble=True,
                                             **dict(kw, batch=5))
    assert np.array_equal(sup5, support) and np.array_equal(got5, got)
    # the grid entry point is the same computation with overlap 0
    tci2, bands2 = np.ascontiguousarray(tci[:, :32]), np.ascontiguousarray(bands[:, :, :32, :])
    tci2 = np.concatenate([tci2, tci2[:, :, :8]], axis=2)                # 32 x 64
    bands2 = np.concatenate([bands2, bands2[:, :, :, :8]], axis=3)
    kw2 = dict(batch=8, bands=bands2, frame_select="clearest", nodata="keep", return_support=True, self_ensemble=True)
    a, sa = super_resolve_scene(model, tci2, n, **kw2)
    b, sb = super_resolve_scene_blended(model, tci2, n, overlap=0, **kw2)
    assert a.shape == (128, 256, 3) and np.array_equal(a, b) and np.array_equal(sa, sb) and sa.max() == n


def test_a_nan_in_any_of_the_eight_outputs_raises():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene_blended
    n = 2
    model = _small_model(3 * n)
    scene = _smooth_scene(43, 4, 32, 32)

    class Poisoned:
        """the generator with a NaN written into row `row` of the plan's output behind every forward"""
        kwargs, compute_dtype = model.kwargs, model.compute_dtype
        row = 0

        def parameters(self):
            return model.parameters()

        def plan_for_inference(self, *a):
            return model.plan_for_inference(*a)

        def run_forward(self, p):
            model.run_forward(p)
            p.out[self.row].view(-1)[0] = float("nan")

    assert super_resolve_scene_blended(model, scene, n, frame_select="clearest", self_ensemble=True).shape == (128, 128, 3)
    for row in (0, 7):                             # the first and the last transform of the one chunk
        bad = Poisoned()
        bad.row = row
        with pytest.raises(FloatingPointError):
            super_resolve_scene_blended(bad, scene, n, frame_select="clearest", self_ensemble=True)


# ---------------------------------------------------------------- 6. unchanged defaults
def test_false_is_the_call_without_the_argument():
    from satlas_super_resolution_amd.infer_scene import super_resolve_scene, super_resolve_scene_blended
    n = 2
    model = _small_model(3 * n)
    for fn, (H, W), kw in ((super_resolve_scene, (32, 64), {}), (super_resolve_scene_blended, (40, 56), {"overlap": 8})):
        scene = _smooth_scene(61, 4, H, W)
        random.seed(6)
        today = fn(model, scene, n, batch=4, **kw).copy()
        random.seed(6)
        got = fn(model, scene, n, batch=4, self_ensemble=False, **kw)
        assert isinstance(got, np.ndarray) and np.array_equal(got, today)
        random.seed(6)
        assert not np.array_equal(fn(model, scene, n, batch=4, self_ensemble=True, **kw), today)


def test_driver_key_absent_is_false_and_true_writes_another_mosaic(tmp_path):
    from PIL import Image
    from satlas_super_resolution_amd.infer_scene import run_infer_scene, super_resolve_scene_blended
    T, H, W, n = 4, 40, 56, 2
    scene = _smooth_scene(62, T, H, W)
    os.makedirs(tmp_path / "scenes")
    Image.fromarray(scene.reshape(T * H, W, 3)).save(tmp_path / "scenes" / "a.png")
    model = _small_model(3 * n)
    opt = {"data_dir": str(tmp_path / "scenes") + "/", "n_lr_images": n, "scene_hw": [H, W], "io_workers": 2, "overlap": 8, "batch": 8}
    files = {}
    for tag, extra in (("absent", {}), ("false", {"self_ensemble": False}), ("true", {"self_ensemble": True})):
        random.seed(9)
        res = run_infer_scene(dict(opt, save_path=str(tmp_path / tag) + "/", **extra), model=model)
        assert (res["scenes"], res["chunks"]) == (1, 4)
        assert ("self_ensemble" in res) == (tag == "true")
        assert _pngs(str(tmp_path / tag)) == ["a/stitched_s2.png", "a/stitched_sr.png"]
        files[tag] = {f: open(tmp_path / tag / "a" / f, "rb").read() for f in ("stitched_s2.png", "stitched_sr.png")}
    assert files["absent"] == files["false"]                              # identical files
    assert files["true"]["stitched_s2.png"] == files["absent"]["stitched_s2.png"]
    sr, sr8 = _png(tmp_path / "absent" / "a" / "stitched_sr.png"), _png(tmp_path / "true" / "a" / "stitched_sr.png")
    assert sr8.shape == sr.shape == (4 * H, 4 * W, 3) and not np.array_equal(sr8, sr)
    assert np.array_equal(_png(tmp_path / "true" / "a" / "stitched_s2.png"), scene[0])
    random.seed(9)
    assert np.array_equal(sr8, super_resolve_scene_blended(model, scene, n, overlap=8, self_ensemble=True))
    with pytest.raises(ValueError, match="self_ensemble"):
        run_infer_scene(dict(opt, save_path=str(tmp_path / "bad") + "/", self_ensemble="yes"), model=model)
