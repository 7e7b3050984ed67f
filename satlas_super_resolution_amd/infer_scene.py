"""Scene inference: one Sentinel-2 image stack in, one super-resolved image out, everything between the upload and the download on
the device.

    python -m satlas_super_resolution_amd.infer_scene -opt infer_scene.yml
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m satlas_super_resolution_amd.infer_scene -opt ...

`infer_grid` keeps the reference's file layout (256 chunk PNGs in, 256 chunk PNGs and two mosaics out, per tile); this driver takes
the image itself: `{data_dir}/NAME.png` of shape [T*H, W, 3] (the T frames stacked on the rows, the chunk files' convention at full
size) or `{data_dir}/NAME.npy` of shape [T, H, W, 3], H and W multiples of 32, and writes `{save_path}/NAME/stitched_sr.png`
([4H, 4W, 3]) and `{save_path}/NAME/stitched_s2.png` (frame 0) - the mosaics `infer_grid` writes for the same pixels.  Every 32 x 32
chunk is super-resolved on its own, as the reference does (ssr/infer_grid.py:46-85), so the result is the reference's mosaic.

On the device (csrc/scene.hip): the "does this frame hold a zero" test of format_s2naip_data for every (chunk, frame), the cut into
chunks + `/ 255` + NHWC straight into the generator plan's input, the generator (a replayed graph), the truncating uint8 + stitch
straight from the plan's output into the mosaic, and the count of non-finite outputs.  On the host: which frames each chunk uses
(`select_scene_frames`: 256 tiny draws that keep the reference's `random` stream), one PNG decode and two encodes per scene, in the
`png_io` worker processes while the device runs another scene.

Option keys: `data_dir`, `save_path`, `n_lr_images`, `network_g`, `path.*`, `compute_dtype` (default fp32h), `batch` (chunks per
generator launch, default 64), `io_workers` as `infer_grid`; `scene_hw: [H, W]` for PNG scenes that are not square; `overlap`;
`s2_bands`; `frame_select`; `nodata`, `nodata_min_support`; `self_ensemble`; `source`, `window`, `reproject_nodata`.

`overlap: K` (0 .. 16; absent: the path above, unchanged) takes scenes of ANY height and width >= 32 instead: chunks overlap their
neighbours by K pixels, the last chunk of a row or column ends at the scene's edge, and the super-resolved chunks are cross-faded
where they overlap (`super_resolve_scene_blended`), which removes the 128-pixel grid that chunks super-resolved alone leave in the
mosaic.  The blend is integer arithmetic on the device, so runs stay bit-identical.

`s2_bands: [tci, b05, b08, ...]` (the dataset's option; absent: the paths above, unchanged) runs multi-band generators, which take
`n_lr_images * (3 + K)` channels: a scene is then the DIRECTORY `{data_dir}/NAME/` with `tci.png` ([T*H, W, 3]) and one 8-bit
grayscale `<band>.png` ([T*H, W]) per extra band - the dataset's `sentinel2/{tile}/{band}.png`, so a split's `sentinel2` folder is a
`data_dir`.  `tci` goes first, the other bands follow in their order, a missing band file contributes zeros, as in
`S2NAIPDataset`; the extra bands take no part in the choice of frames.  `super_resolve_scene(_blended)(..., bands=)` takes them as
uint8 [K, T, H, W].

`frame_select: random | clearest` (absent: `random`, the paths above, unchanged) is the frame policy.  `random` is the reference's
rule (`select_scene_frames`).  `clearest` is this project's own policy - the reference has no counterpart file - computed on the
device (`ssr_scene_frame_keys`, `ssr_scene_rank_frames`): per chunk the `n_lr_images` frames with the fewest NODATA pixels (a zero
sample), then the fewest saturated ones (255, 255, 255: clouds, snow, glint), then the lower index, best frame first
(`rank_scene_frames`).  Every frame without a zero precedes every frame with one, so the chosen set is always one the reference's
rule could have drawn.  It is deterministic, does not touch the `random` module and leaves no host round trip between the upload
and the download of the mosaic.  It works with `overlap` and `s2_bands` (the keys are computed on the TCI alone); `stitched_s2.png`
stays frame 0 under both policies.

`nodata: fill | keep` (absent: `fill`, the paths above, unchanged byte for byte and launch for launch) is what becomes of ESA's
NODATA (the value 0 of the TCI).  Under `fill` the generator runs on the zeros and whatever it makes of them is written as imagery,
as the reference does.  `keep` is this project's own policy - the reference has no counterpart file: NODATA in, NODATA out.  A
low-resolution pixel of a frame HAS DATA if none of its three TCI samples is 0 (the complement of the `z` count of
`ssr_scene_frame_keys`; the extra bands of `s2_bands` take no part).  `support[y, x]` is the number of pairs (chunk that covers
(y, x), chosen frame slot of that chunk) whose TCI pixel at (y, x) has data - exactly what went into the generator
(`scene_support`).  With `nodata_min_support: m` (an integer >= 1, default 1) every sample of the 4 x 4 output block of a pixel with
support < m becomes 0, every other sample max(1, sample): 0 stays reserved for NODATA in the output (`apply_nodata`).  The driver
then writes a third file, `{save_path}/NAME/stitched_support.png`: min(support, 255), 8-bit grayscale [H, W].  All of it is integer
work on the device (`ssr_scene_support_add`, `ssr_scene_apply_nodata`) between the upload and the one download, which grows by
H W bytes; it works with `overlap`, `s2_bands` and both frame policies.

`self_ensemble: true | false` (absent: false, the paths above, unchanged byte for byte and launch for launch) is BasicSR's
`val.self_ensemble` (`SRModel.test_selfensemble`; the reference's model overrides `test`, so it never offers it) over chunks: every
chunk goes through the generator under the eight flips and transposes of the square and the eight outputs are turned back and
averaged, which takes away the orientation-dependent texture a GAN generator invents - satellite imagery has no preferred orientation.
The transform set is BasicSR's ('v', 'h', 't': here bit 0 of the transform id flips the columns, bit 1 the rows, bit 2 transposes;
`ensemble_transform`, `ensemble_inverse` state them).  The averaging is NOT BasicSR's float mean but this project's integer blend, so
the bytes are not BasicSR's: each of the eight outputs in 13-bit fixed point ((uint32) (clamp(v, 0, 1) * 8191.0f) - eight rows per
chunk would overflow the accumulator at the blend's 16 bits), times the blend window, into the same uint32 accumulator, and
mosaic = acc * 255 // (8 * Sy * Sx * 8191).  It always runs on the accumulator path: with `overlap` as documented above, without it
as overlap 0 (sizes still multiples of 32).  The generator's rows are the (chunk, transform) pairs in chunk-major order and `batch`
slices that list, so a scene takes eight times the generator time; the frames of a chunk are chosen once, as without the option
(`random` is consumed once per chunk), `nodata` and the support map are what they are without it.  On the device:
`ssr_scene_gather_tf` writes a transformed chunk into the plan's input, `ssr_scene_blend_add_tf` turns the output back while it
accumulates, `ssr_scene_blend_finish_scaled` divides.  Integer sums: the bytes do not depend on `batch`, and with `frame_select:
clearest` and chunk origins symmetric about the centre the mosaic of a flipped or transposed scene is the flipped or transposed mosaic,
byte for byte.

`source: sentinel2_l1c` (absent: every path above, launch for launch; nothing new runs) starts from what ESA ships instead of stacks
that already lie on the grid: a scene is the DIRECTORY `{data_dir}/NAME/` of T products sorted by name - `.SAFE` directories (their
`*_TCI.jp2` under GRANULE/*/IMG_DATA/, georeferenced by GRANULE/*/MTD_TL.xml) or raster files (.jp2 / .tif / .png / .npy) with a
sidecar NAME.json - in UTM.  `window: {tile: "COL_ROW", zoom: 13 | 17} | {pixels: [px0, py0, w, h]} | {bbox: [lon_min, lat_min,
lon_max, lat_max]}` names the pixels of the model's Web-Mercator grid to produce (multiples of 32, at most 4096 per side);
`reproject_nodata: blend | propagate` (default `blend`) is what a zero sample does in the bilinear warp.  `s2_reproject.py` states the
grid, the projection and the warp for the CPU and is their definition - the bytes are NOT GDAL's, which the reference's pseudo-code
would call.  Per scene the `png_io` workers decode the rasters (Pillow: JPEG 2000, TIFF) and keep only the rectangle the window
needs; on the device `ssr_merc_to_utm_coords` computes one coordinate array per distinct georeference and `ssr_scene_warp_bilinear`
warps the frames into one tensor uint8 [T, h, w, 3], which goes to the paths above as it is (`reproject_scene` in Python).  It works
with `overlap`, `frame_select`, `nodata` and `self_ensemble`; `s2_bands` beside it is refused by name (the 16-bit band files are out
of scope).  `stitched_s2.png` is the reprojected frame 0; `stitched_sr.json` / `stitched_s2.json` hold EPSG 3857, the upper-left
corner in metres, the pixel size and the window in global pixels."""
from __future__ import annotations

import argparse
import os
import random
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

CHUNK = 32            # low-resolution chunk edge (format_s2naip_data)
SCALE = 4


# ------------------------------------------------------------------------------------------------ host side
def select_scene_frames(has_zero: np.ndarray, n: int) -> np.ndarray:
    """Which frames of every chunk go to the network: has_zero bool [chunks, T] (does frame t of the chunk hold a zero sample) ->
    int32 [chunks, n].  `utils.infer_utils.select_frames`' rule per chunk - clean frames are preferred, frames that hold zeros top
    the list up, fewer than n frames in total make `random.sample` raise ValueError - with the `random` module consumed once per
    chunk in ROW-MAJOR chunk order: a seeded run picks what format_s2naip_data would pick called on the chunks in that order."""
    has_zero = np.asarray(has_zero).astype(bool)
    assert has_zero.ndim == 2, has_zero.shape
    out = np.empty((has_zero.shape[0], n), np.int32)
    for k, hz in enumerate(has_zero):
        clean, dirty = np.flatnonzero(~hz).tolist(), np.flatnonzero(hz).tolist()
        if len(clean) >= n:
            out[k] = random.sample(clean, n)
        else:
            out[k] = clean + random.sample(dirty, n - len(clean))
    return out


FRAME_POLICIES = ("random", "clearest")
MAX_SELECT_FRAMES = 1024      # frames per scene ssr_scene_rank_frames ranks (its LDS holds a chunk's keys)


def rank_scene_frames(z: np.ndarray, s: np.ndarray, n: int) -> np.ndarray:
    """The `clearest` policy restated in numpy (the inference path computes it on the device: `scene_frame_keys`,
    `scene_rank_frames`).  z, s: integers [chunks, T], per frame t of a chunk's 32 x 32 TCI window the number of pixels with AT LEAST
    ONE zero sample (ESA's NODATA) and the number whose three samples are ALL 255 (SATURATED: clouds, snow, glint) -> int32
    [chunks, n]: the first n frames in the order (key, t) ascending, key = (z << 16) | s - fewest NODATA pixels first, then fewest
    saturated ones, then the lower frame index - best frame first.  ValueError if n > T.
    z > 0 is `select_scene_frames`' has_zero flag and z leads the key, so every frame without a zero precedes every frame with one:
    the chosen set is all the clean frames topped up with dirty ones if there are fewer than n, otherwise n clean ones - always a
    set the reference's rule could have drawn.  Nothing is drawn: the `random` module is not consumed."""
    z, s = np.asarray(z), np.asarray(s)
    assert z.ndim == 2 and z.shape == s.shape, (z.shape, s.shape)
    n = int(n)
    if not 1 <= n <= z.shape[1]:
        raise ValueError(f"n_lr_images = {n} frames of a scene of {z.shape[1]}")
    key = (z.astype(np.uint32) << np.uint32(16)) | s.astype(np.uint32)
    return np.argsort(key, axis=1, kind="stable")[:, :n].astype(np.int32)      # stable: the lower index wins a tie


def check_frame_select(frame_select, T: Optional[int] = None, n: Optional[int] = None) -> str:
    """the refusals of a frame policy, all on the host: a value other than `random` / `clearest`; for `clearest`, given T and n,
    more frames than the ranking kernel takes and fewer frames than are asked for (where `random.sample` raises under `random`)"""
    if frame_select not in FRAME_POLICIES:
        raise ValueError(f"frame_select = {frame_select!r}: one of {', '.join(FRAME_POLICIES)}")
    if frame_select == "clearest" and T is not None:
        if T > MAX_SELECT_FRAMES:
            raise ValueError(f"frame_select: clearest ranks at most {MAX_SELECT_FRAMES} frames per scene, this one has {T}")
        if n is not None and not 1 <= n <= T:
            raise ValueError(f"n_lr_images = {n} frames of a scene of {T}")
    return frame_select


NODATA_POLICIES = ("fill", "keep")


def scene_support(tci: np.ndarray, origins, frame_ids) -> np.ndarray:
    """The support map of the `nodata: keep` policy restated in numpy - the statement of the policy (the inference path computes
    it on the device: `scene_support_add`).  tci uint8 [T, H, W, 3], origins integers [B, 2] (y0, x0), frame_ids integers [B, n] ->
    int32 [H, W]: support[y, x] = the number of pairs (chunk b whose 32 x 32 window covers (y, x), slot k < n) whose TCI pixel
    tci[frame_ids[b, k], y, x] HAS DATA, that is none of its three samples is 0 (ESA's NODATA; the complement of the `z` count of
    `rank_scene_frames`).  It counts exactly what went into the generator: a chunk whose origin lies outside the scene or one of
    whose frame ids lies outside 0 .. T - 1 contributes nothing - the gather kernels make such a chunk a no-op too.  A frame that
    fills two slots counts twice.  On the grid path support <= n, on the blended path up to 3 chunks per axis cover a pixel
    (`scene_chunk_origins(52, 16)` = [0, 16, 20]): support <= 9 n."""
    tci = np.asarray(tci)
    assert tci.dtype == np.uint8 and tci.ndim == 4 and tci.shape[3] == 3, (tci.dtype, tci.shape)
    origins, frame_ids = np.asarray(origins).reshape(-1, 2), np.asarray(frame_ids)
    assert frame_ids.ndim == 2 and frame_ids.shape[0] == origins.shape[0], (origins.shape, frame_ids.shape)
    T, H, W = tci.shape[:3]
    data = (tci != 0).all(axis=-1)
    support = np.zeros((H, W), np.int32)
    for (y0, x0), ids in zip(origins.tolist(), frame_ids):
        if not (0 <= y0 <= H - CHUNK and 0 <= x0 <= W - CHUNK) or (ids < 0).any() or (ids >= T).any():
            continue
        support[y0:y0 + CHUNK, x0:x0 + CHUNK] += data[ids, y0:y0 + CHUNK, x0:x0 + CHUNK].sum(axis=0, dtype=np.int32)
    return support


def apply_nodata(mosaic: np.ndarray, support: np.ndarray, min_support: int = 1) -> np.ndarray:
    """The output rule of the `nodata: keep` policy restated in numpy - the statement of the policy (on the device:
    `scene_apply_nodata`).  mosaic uint8 [4H, 4W, C], support integers [H, W] (`scene_support`) -> uint8 [4H, 4W, C]: every sample of
    the 4 x 4 output block of a low-resolution pixel becomes 0 where support < min_support and max(1, sample) where support >=
    min_support: 0 stays reserved for NODATA in the output, as it is in ESA's input."""
    mosaic, support = np.asarray(mosaic), np.asarray(support)
    assert mosaic.dtype == np.uint8 and mosaic.ndim == 3 and support.ndim == 2, (mosaic.dtype, mosaic.shape, support.shape)
    assert mosaic.shape[:2] == (SCALE * support.shape[0], SCALE * support.shape[1]), (mosaic.shape, support.shape)
    _, m = check_nodata("keep", min_support)
    up = np.repeat(np.repeat(support, SCALE, axis=0), SCALE, axis=1)[:, :, None]
    return np.where(up < m, 0, np.maximum(mosaic, 1)).astype(np.uint8)


def support_to_u8(support: np.ndarray) -> np.ndarray:
    """the support map as it comes back with the mosaic: uint8 [H, W], min(support, 255)"""
    return np.minimum(np.asarray(support), 255).astype(np.uint8)


def check_nodata(nodata, min_support=1) -> Tuple[str, int]:
    """the refusals of the NODATA option, all on the host: a value other than `fill` / `keep`; a min_support that is not an
    integer >= 1; a min_support other than 1 together with `fill`, which has no support map to compare it with"""
    if not isinstance(nodata, str) or nodata not in NODATA_POLICIES:
        raise ValueError(f"nodata = {nodata!r}: one of {', '.join(NODATA_POLICIES)}")
    if isinstance(min_support, bool) or not isinstance(min_support, (int, np.integer)) or min_support < 1:
        raise ValueError(f"min_support = {min_support!r}: an integer >= 1")
    if min_support >= 1 << 31:
        raise ValueError(f"min_support = {min_support!r}: an integer below 2^31")
    if nodata == "fill" and min_support != 1:
        raise ValueError(f"min_support = {min_support} has a meaning under nodata: keep only (nodata = 'fill')")
    return nodata, int(min_support)


ENSEMBLE = 8                  # the symmetries of the square: the rows a chunk takes in the generator under `self_ensemble`
ENSEMBLE_ONE = 8191           # 1.0 in the self-ensemble's fixed point: 13 fractional bits (8 * 125 * 125 * 8191 < 2^32)


def ensemble_transform(P: np.ndarray, tf: int) -> np.ndarray:
    """The self-ensemble's transform tf (0 .. 7) of a chunk restated in numpy - the statement of the option (the inference path
    computes it on the device: `scene_gather_tf`).  P: an array whose first two axes are the chunk's rows and columns ([32, 32, C_in]
    going into the generator); the channel axis is untouched.  Bit 0 of tf flips the columns, bit 1 flips the rows, bit 2
    transposes, applied in that order: the eight symmetries of the square, the set of BasicSR's `val.self_ensemble`
    (SRModel.test_selfensemble: 'v', 'h', 't')."""
    tf = int(tf)
    if not 0 <= tf < ENSEMBLE:
        raise ValueError(f"tf = {tf}: a transform id from 0 to {ENSEMBLE - 1}")
    A = np.asarray(P)
    if tf & 1:
        A = A[:, ::-1]
    if tf & 2:
        A = A[::-1]
    if tf & 4:
        A = A.swapaxes(0, 1)
    return A


def ensemble_inverse(O: np.ndarray, tf: int) -> np.ndarray:
    """What undoes `ensemble_transform(., tf)`: the bits in the opposite order (on the device: `scene_blend_add_tf`, which turns a
    [128, 128, C_out] output back while it accumulates).  ensemble_inverse(ensemble_transform(P, tf), tf) == P."""
    tf = int(tf)
    if not 0 <= tf < ENSEMBLE:
        raise ValueError(f"tf = {tf}: a transform id from 0 to {ENSEMBLE - 1}")
    A = np.asarray(O)
    if tf & 4:
        A = A.swapaxes(0, 1)
    if tf & 2:
        A = A[::-1]
    if tf & 1:
        A = A[:, ::-1]
    return A


def check_self_ensemble(self_ensemble) -> bool:
    """the refusal of the self-ensemble option, on the host: anything but a bool"""
    if not isinstance(self_ensemble, (bool, np.bool_)):
        raise ValueError(f"self_ensemble = {self_ensemble!r}: true or false")
    return bool(self_ensemble)


def check_scene_size(H: int, W: int, any_size: bool = False) -> None:
    if any_size:
        if H < CHUNK or W < CHUNK:
            raise ValueError(f"scene of {H} x {W} pixels: height and width must be at least {CHUNK}")
    elif H <= 0 or W <= 0 or H % CHUNK or W % CHUNK:
        raise ValueError(f"scene of {H} x {W} pixels: height and width must be multiples of {CHUNK}")


MAX_OVERLAP = CHUNK // 2
SR_CHUNK = SCALE * CHUNK


def scene_chunk_origins(L: int, overlap: int) -> List[int]:
    """Where the 32-pixel chunks of the blended path start along an axis of L low-resolution pixels: 0, s, 2s, ... with the stride
    s = 32 - overlap for as long as origin + 32 < L, then L - 32 (the last chunk ends at the scene's edge and overlaps its
    neighbour by whatever is left).  0 <= overlap <= 16 and L >= 32, ValueError otherwise."""
    L, ov = int(L), int(overlap)
    if ov != overlap or not 0 <= ov <= MAX_OVERLAP:
        raise ValueError(f"overlap = {overlap}: an integer from 0 to {MAX_OVERLAP}")
    if L < CHUNK:
        raise ValueError(f"a scene axis of {L} pixels is shorter than a chunk ({CHUNK})")
    out, o = [], 0
    while o + CHUNK < L:
        out.append(o)
        o += CHUNK - ov
    return out + [L - CHUNK]


def scene_chunk_grid(H: int, W: int, overlap: int) -> np.ndarray:
    """int32 [chunks, 2]: (y0, x0) of every chunk, the cross product of the row and the column origins in row-major order"""
    ys, xs = scene_chunk_origins(H, overlap), scene_chunk_origins(W, overlap)
    return np.array([(y, x) for y in ys for x in xs], np.int32).reshape(-1, 2)


def blend_window(overlap: int) -> np.ndarray:
    """int32 [128]: the weight of row (or column) r of a super-resolved chunk, w[r] = min(r + 1, 128 - r, R), R = max(1, 4 overlap);
    a sample's weight is w[r] * w[c].  Where two chunks overlap by `overlap` pixels the two ramps add up to R + 1: a linear
    cross-fade.  Nothing is special at a scene edge: the division by the sum of the weights makes a lone chunk's sample itself."""
    scene_chunk_origins(CHUNK, overlap)             # (the range check)
    r = np.arange(SR_CHUNK)
    return np.minimum(np.minimum(r + 1, SR_CHUNK - r), max(1, SCALE * int(overlap))).astype(np.int32)


def blend_weight_sums(L: int, overlap: int) -> np.ndarray:
    """int32 [4 L]: for every output row (column) the sum of `blend_window` over the chunks that cover it (>= 1, <= 125)"""
    w = blend_window(overlap)
    S = np.zeros(SCALE * int(L), np.int32)
    for o in scene_chunk_origins(L, overlap):
        S[SCALE * o:SCALE * o + SR_CHUNK] += w
    return S


def parse_scene(arr: np.ndarray, scene_hw: Optional[Sequence[int]] = None, any_size: bool = False) -> np.ndarray:
    """A scene file's array -> uint8 [T, H, W, 3].  [T, H, W, 3] (.npy) is taken as it is; [T*H, W, 3] (.png: the frames stacked on
    the rows) is cut with H = scene_hw[0] (and W checked against scene_hw[1]) or, without scene_hw, as square frames H = W.  H and W
    are multiples of 32, or with any_size (the blended path) anything from 32 up."""
    arr = np.asarray(arr)
    if arr.dtype != np.uint8 or arr.ndim not in (3, 4) or arr.shape[-1] != 3:
        raise ValueError(f"a scene is a uint8 array [T, H, W, 3] or [T*H, W, 3], not {arr.dtype} {tuple(arr.shape)}")
    if arr.ndim == 3:
        rows, W = arr.shape[:2]
        H = W
        if scene_hw is not None:
            H = int(scene_hw[0])
            if int(scene_hw[1]) != W:
                raise ValueError(f"scene image of {rows} x {W} pixels: scene_hw {list(scene_hw)} expects width {int(scene_hw[1])}")
        if H <= 0 or rows % H or rows == 0:
            raise ValueError(f"scene image of {rows} x {W} pixels: {rows} rows are not a whole number of frames of height {H}"
                             + ("" if scene_hw is not None else " (square frames are assumed: set scene_hw: [H, W])"))
        arr = arr.reshape(rows // H, H, W, 3)
    check_scene_size(arr.shape[1], arr.shape[2], any_size)
    return arr


def list_scenes(data_dir: str) -> List[Tuple[str, str]]:
    """[(NAME, path)] of the scene files of data_dir (NAME.png / NAME.npy), sorted by NAME"""
    found = {}
    for f in os.listdir(data_dir):
        name, ext = os.path.splitext(f)
        if ext.lower() in (".png", ".npy") and os.path.isfile(os.path.join(data_dir, f)):
            if name in found:
                raise ValueError(f"{data_dir}: scene {name!r} exists as both {os.path.basename(found[name])} and {f}")
            found[name] = os.path.join(data_dir, f)
    return sorted(found.items())


def order_s2_bands(bands: Sequence[str]) -> List[str]:
    """`s2_bands` as the dataset orders it (data/s2naip_dataset.py): `tci`, which is required, first, the rest in their order"""
    bands = [str(b) for b in bands]
    if "tci" not in bands:
        raise ValueError(f"s2_bands = {bands}: 'tci' is required")
    bands.insert(0, bands.pop(bands.index("tci")))
    return bands


def list_band_scenes(data_dir: str, bands: Sequence[str]) -> List[Tuple[str, str, List[Optional[str]]]]:
    """[(NAME, path of tci.png, [path of <band>.png or None where the file is missing, per extra band])] of the scene directories
    `data_dir/NAME/` (those that hold a tci.png), sorted by NAME; bands as `s2_bands` (any order, `tci` among them)"""
    extra = order_s2_bands(bands)[1:]
    out = []
    for name in sorted(os.listdir(data_dir)):
        tci = os.path.join(data_dir, name, "tci.png")
        if os.path.isfile(tci):
            paths = [os.path.join(data_dir, name, b + ".png") for b in extra]
            out.append((name, tci, [p if os.path.isfile(p) else None for p in paths]))
    return out


def band_scene_shape(tci_path: str, band_paths: Sequence[Optional[str]]) -> Tuple[int, int]:
    """(rows, W) of a band scene's tci.png, from the files' headers; ValueError naming the file for a band file of another size or
    one that is not 8-bit grayscale"""
    from PIL import Image
    rows, W, _ = _png_shape(tci_path)
    for p in band_paths:
        if p is None:
            continue
        with Image.open(p) as im:          # header only
            (w, h), mode = im.size, im.mode
        if mode != "L":
            raise ValueError(f"{p}: a band file is an 8-bit grayscale PNG, not mode {mode!r}")
        if (h, w) != (rows, W):
            raise ValueError(f"{p}: {h} x {w} pixels, {os.path.basename(tci_path)} beside it has {rows} x {W}")
    return rows, W


SOURCES = ("sentinel2_l1c",)


def check_source(source, s2_bands=None) -> Optional[str]:
    """the refusals of the `source` option, on the host: a value other than `sentinel2_l1c`; `s2_bands` beside it (the 16-bit band
    files and their / 8160 scaling are out of scope)"""
    if source is None:
        return None
    if source not in SOURCES:
        raise ValueError(f"source = {source!r}: one of {', '.join(SOURCES)} (absent: scenes that already lie on the grid)")
    if s2_bands is not None:
        raise ValueError(f"s2_bands = {list(s2_bands)} with source: {source}: the 16-bit band files of an L1C product are not read; "
                         "this source takes the TCI alone")
    return source


def list_product_scenes(data_dir: str) -> List[Tuple[str, List[str]]]:
    """[(NAME, its products sorted by name)] of the scene directories `data_dir/NAME/` that hold at least one product (a `.SAFE`
    directory or a raster file with its sidecar), sorted by NAME"""
    from .s2_reproject import list_products
    out = []
    for name in sorted(os.listdir(data_dir)):
        d = os.path.join(data_dir, name)
        if os.path.isdir(d) and not name.upper().endswith(".SAFE"):
            products = list(list_products(d))
            if products:
                out.append((name, products))
    return out


def scenes_of_rank(scenes: Sequence, rank: int, world: int) -> List:
    """rank r takes scenes r, r + world, ... of the sorted list (no collective, no barrier: every scene is one rank's own)"""
    return list(scenes[rank::world])


def _png_shape(path: str) -> Tuple[int, int, int]:
    from PIL import Image
    with Image.open(path) as im:          # header only: nothing is decoded here
        w, h = im.size
    return (h, w, 3)


# ------------------------------------------------------------------------------------------------ device side
def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _check_scene(scene: torch.Tensor, any_size: bool = False) -> Tuple[int, int, int]:
    """a scene (the TCI) on the device, uint8 [T, H, W, 3] of a size the path takes -> (T, H, W)"""
    assert scene.is_cuda and scene.dtype == torch.uint8 and scene.is_contiguous() and scene.dim() == 4 and scene.shape[3] == 3, \
        (scene.dtype, scene.shape)
    T, H, W = scene.shape[:3]
    check_scene_size(H, W, any_size)
    return T, H, W


def _check_origins(origins: torch.Tensor):
    assert origins.is_cuda and origins.dtype == torch.int32 and origins.is_contiguous() and origins.dim() == 2 and origins.shape[1] == 2, \
        (origins.dtype, origins.shape)


def _check_frame_ids(frame_ids: torch.Tensor, origins: torch.Tensor) -> Tuple[int, int]:
    """the chosen frames of the chunks at the origins, int32 [B, n] on the device -> (B, n)"""
    _check_origins(origins)
    assert frame_ids.is_cuda and frame_ids.dtype == torch.int32 and frame_ids.is_contiguous() and frame_ids.dim() == 2 \
        and frame_ids.shape[0] == origins.shape[0], (frame_ids.dtype, frame_ids.shape, origins.shape)
    return tuple(frame_ids.shape)


def _check_bands_tensor(bands: Optional[torch.Tensor], T: int, H: int, W: int) -> int:
    """the extra bands of a scene on the device, uint8 [K, T, H, W], or None -> K"""
    if bands is None:
        return 0
    assert bands.is_cuda and bands.dtype == torch.uint8 and bands.is_contiguous() and bands.dim() == 4 and bands.shape[0] >= 1 \
        and tuple(bands.shape[1:]) == (T, H, W), (bands.dtype, bands.shape, (T, H, W))
    return bands.shape[0]


def _check_tf(tf: torch.Tensor, B: int):
    assert tf.is_cuda and tf.dtype == torch.int32 and tf.is_contiguous() and tuple(tf.shape) == (B,), (tf.dtype, tf.shape)


def _check_acc(acc: torch.Tensor, C: int):
    assert acc.is_cuda and acc.dtype == torch.int32 and acc.is_contiguous() and acc.dim() == 3 and acc.shape[2] == C, (acc.dtype, acc.shape)


def scene_zero_scan(scene: torch.Tensor) -> torch.Tensor:
    """uint8 [T, H, W, 3] on the device -> uint8 [gh*gw, T] on the device: 1 where frame t of the chunk holds a zero sample"""
    from . import hip
    T, H, W = _check_scene(scene)
    out = torch.empty((H // CHUNK) * (W // CHUNK), T, dtype=torch.uint8, device=scene.device)
    hip.check(hip.lib().ssr_scene_zero_scan(_ptr(scene), T, H, W, _ptr(out), hip.stream_ptr()), "ssr_scene_zero_scan")
    return out


def scene_gather(scene: torch.Tensor, chunk_ids: torch.Tensor, frame_ids: torch.Tensor, dst: torch.Tensor, dtype: Optional[int] = None):
    """the chosen frames (int32 [B, n], device) of the chunks chunk_ids (int32 [B], device) -> dst, an NHWC generator input
    [B, 32, 32, >= 3n] of fp32 or bf16 storage (GeneratorPlan.xin); pad channels are left as they are"""
    from . import hip
    assert chunk_ids.dtype == torch.int32 and frame_ids.dtype == torch.int32 and chunk_ids.is_cuda and frame_ids.is_cuda
    assert chunk_ids.is_contiguous() and frame_ids.is_contiguous()
    T, H, W = _check_scene(scene)
    B, n = frame_ids.shape
    assert chunk_ids.shape == (B,) and tuple(dst.shape[:3]) == (B, CHUNK, CHUNK) and dst.shape[3] >= 3 * n, (chunk_ids.shape, dst.shape)
    if dtype is None:
        dtype = hip.dtype_code(dst.dtype)
    hip.check(hip.lib().ssr_scene_gather(_ptr(scene), T, H, W, _ptr(chunk_ids), _ptr(frame_ids), B, n, hip.view(dst), dtype,
                                         hip.stream_ptr()), "ssr_scene_gather")


def scene_scatter_u8(src: torch.Tensor, chunk_ids: torch.Tensor, C: int, mosaic: torch.Tensor, nonfinite: torch.Tensor,
                     dtype: Optional[int] = None):
    """src, an NHWC generator output [B, 128, 128, >= C] (GeneratorPlan.out) -> truncating uint8 at the places of the chunks
    chunk_ids in mosaic (uint8 [Ho, Wo, C], device); adds the number of non-finite samples to the int32 device counter"""
    from . import hip
    B = chunk_ids.shape[0]
    assert chunk_ids.dtype == torch.int32 and chunk_ids.is_cuda and chunk_ids.is_contiguous()
    assert tuple(src.shape[:3]) == (B, SCALE * CHUNK, SCALE * CHUNK) and src.shape[3] >= C, src.shape
    assert mosaic.is_cuda and mosaic.dtype == torch.uint8 and mosaic.is_contiguous() and mosaic.dim() == 3 and mosaic.shape[2] == C
    assert nonfinite.dtype == torch.int32 and nonfinite.is_cuda
    if dtype is None:
        dtype = hip.dtype_code(src.dtype)
    hip.check(hip.lib().ssr_scene_scatter_u8(hip.view(src), dtype, _ptr(chunk_ids), B, C, _ptr(mosaic), mosaic.shape[0],
                                             mosaic.shape[1], _ptr(nonfinite), hip.stream_ptr()), "ssr_scene_scatter_u8")


def scene_zero_scan_at(scene: torch.Tensor, origins: torch.Tensor) -> torch.Tensor:
    """uint8 [T, H, W, 3] (H, W >= 32) and int32 [chunks, 2] origins (y0, x0), both on the device -> uint8 [chunks, T] on the device:
    1 where frame t of the 32 x 32 window at the origin holds a zero sample; rows of origins outside the scene are not written"""
    from . import hip
    T, H, W = _check_scene(scene, True)
    _check_origins(origins)
    out = torch.zeros(origins.shape[0], T, dtype=torch.uint8, device=scene.device)
    hip.check(hip.lib().ssr_scene_zero_scan_at(_ptr(scene), T, H, W, _ptr(origins), origins.shape[0], _ptr(out), hip.stream_ptr()),
              "ssr_scene_zero_scan_at")
    return out


def scene_frame_keys(scene: torch.Tensor, origins: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [T, H, W, 3] (H, W >= 32, the TCI) and int32 [chunks, 2] origins (y0, x0), both on the device -> int32 storage [chunks, T]
    on the device, read as uint32: (z << 16) | s of frame t of the 32 x 32 window at the origin, z its pixels with at least one zero
    sample, s its pixels that are (255, 255, 255) (`rank_scene_frames`); rows of origins outside the scene are not written (they
    keep what `out` held, zeros without one)"""
    from . import hip
    T, H, W = _check_scene(scene, True)
    _check_origins(origins)
    if out is None:
        out = torch.zeros(origins.shape[0], T, dtype=torch.int32, device=scene.device)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (origins.shape[0], T), (out.dtype, out.shape)
    hip.check(hip.lib().ssr_scene_frame_keys(_ptr(scene), T, H, W, _ptr(origins), origins.shape[0], _ptr(out), hip.stream_ptr()),
              "ssr_scene_frame_keys")
    return out


def scene_rank_frames(keys: torch.Tensor, n: int) -> torch.Tensor:
    """keys (int32 storage [chunks, T] on the device, read as uint32: `scene_frame_keys`) -> int32 [chunks, n] on the device, the
    frame_ids the gathers read: per chunk the first n frames in the order (key, frame index) ascending, exact and the same in every
    run.  ValueError for more than 1024 frames and for n > T."""
    from . import hip
    assert keys.dtype == torch.int32 and keys.dim() == 2 and keys.shape[0] >= 1, (keys.dtype, keys.shape)
    chunks, T = keys.shape
    n = int(n)
    check_frame_select("clearest", T, n)
    assert keys.is_cuda and keys.is_contiguous()
    out = torch.empty(chunks, n, dtype=torch.int32, device=keys.device)
    hip.check(hip.lib().ssr_scene_rank_frames(_ptr(keys), chunks, T, n, _ptr(out), hip.stream_ptr()), "ssr_scene_rank_frames")
    return out


def _gather_at(scene: torch.Tensor, bands: Optional[torch.Tensor], origins: torch.Tensor, frame_ids: torch.Tensor,
               tf: Optional[torch.Tensor], dst: torch.Tensor, dtype: Optional[int]):
    """the body of the three gathers at origins: `ssr_scene_gather_tf` with transform ids, else `ssr_scene_gather_bands` with bands,
    else `ssr_scene_gather_at`"""
    from . import hip
    T, H, W = _check_scene(scene, True)
    K = _check_bands_tensor(bands, T, H, W)
    B, n = _check_frame_ids(frame_ids, origins)
    assert tuple(dst.shape[:3]) == (B, CHUNK, CHUNK) and dst.shape[3] >= (3 + K) * n, (origins.shape, dst.shape)
    if dtype is None:
        dtype = hip.dtype_code(dst.dtype)
    tail = (B, n, hip.view(dst), dtype, hip.stream_ptr())
    if tf is not None:
        _check_tf(tf, B)
        hip.check(hip.lib().ssr_scene_gather_tf(_ptr(scene), None if bands is None else _ptr(bands), K, T, H, W, _ptr(origins),
                                                _ptr(frame_ids), _ptr(tf), *tail), "ssr_scene_gather_tf")
    elif bands is not None:
        hip.check(hip.lib().ssr_scene_gather_bands(_ptr(scene), _ptr(bands), K, T, H, W, _ptr(origins), _ptr(frame_ids), *tail),
                  "ssr_scene_gather_bands")
    else:
        hip.check(hip.lib().ssr_scene_gather_at(_ptr(scene), T, H, W, _ptr(origins), _ptr(frame_ids), *tail), "ssr_scene_gather_at")


def scene_gather_at(scene: torch.Tensor, origins: torch.Tensor, frame_ids: torch.Tensor, dst: torch.Tensor, dtype: Optional[int] = None):
    """`scene_gather` for chunks at the origins (int32 [B, 2], device) of a scene of any size >= 32 x 32"""
    _gather_at(scene, None, origins, frame_ids, None, dst, dtype)


def scene_gather_bands(scene: torch.Tensor, bands: torch.Tensor, origins: torch.Tensor, frame_ids: torch.Tensor, dst: torch.Tensor,
                       dtype: Optional[int] = None):
    """`scene_gather_at` with the K extra bands (uint8 [K, T, H, W], device) behind the TCI of every chosen frame: 3 + K channels
    per frame, dst [B, 32, 32, >= n (3 + K)]"""
    assert bands is not None
    _gather_at(scene, bands, origins, frame_ids, None, dst, dtype)


def scene_gather_tf(scene: torch.Tensor, bands: Optional[torch.Tensor], origins: torch.Tensor, frame_ids: torch.Tensor,
                    tf: torch.Tensor, dst: torch.Tensor, dtype: Optional[int] = None):
    """`ensemble_transform` on the device: row b of dst is the transform tf[b] (int32 [B], device) of the chunk `scene_gather_at`
    (bands None) or `scene_gather_bands` writes for origins[b] and frame_ids[b] - with tf[b] == 0 their bytes.  A row whose tf lies
    outside 0 .. 7 is left as it is, as a row they skip."""
    assert tf is not None
    _gather_at(scene, bands, origins, frame_ids, tf, dst, dtype)


def scene_support_add(scene: torch.Tensor, origins: torch.Tensor, frame_ids: torch.Tensor, support: torch.Tensor):
    """`scene_support` on the device, for the chunks at the origins (int32 [B, 2], device) with the chosen frames frame_ids (int32
    [B, n], device) - the arguments of the gather beside it: per pixel of every chunk's window the number of slots whose TCI pixel
    has data (no zero sample) is ADDED to support (int32 [H, W], device; the caller zeroes it once per scene).  Chunks the gathers
    skip (origin outside the scene, a frame id outside 0 .. T - 1) add nothing."""
    from . import hip
    T, H, W = _check_scene(scene, True)
    B, n = _check_frame_ids(frame_ids, origins)
    assert support.is_cuda and support.dtype == torch.int32 and support.is_contiguous() and tuple(support.shape) == (H, W), \
        (support.dtype, support.shape)
    hip.check(hip.lib().ssr_scene_support_add(_ptr(scene), T, H, W, _ptr(origins), _ptr(frame_ids), B, n, _ptr(support),
                                              hip.stream_ptr()), "ssr_scene_support_add")


def scene_apply_nodata(mosaic: torch.Tensor, support: torch.Tensor, min_support: int = 1, support_u8: Optional[torch.Tensor] = None):
    """`apply_nodata` on the device, in place: mosaic uint8 [4H, 4W, C] and support int32 [H, W], both on the device - samples of
    pixels with support < min_support become 0, all others max(1, sample); support_u8 (uint8 [H, W], device), if given, receives
    min(support, 255)"""
    from . import hip
    assert mosaic.is_cuda and mosaic.dtype == torch.uint8 and mosaic.is_contiguous() and mosaic.dim() == 3, (mosaic.dtype, mosaic.shape)
    Ho, Wo, C = mosaic.shape
    assert Ho % SCALE == 0 and Wo % SCALE == 0, mosaic.shape
    H, W = Ho // SCALE, Wo // SCALE
    assert support.is_cuda and support.dtype == torch.int32 and support.is_contiguous() and tuple(support.shape) == (H, W), \
        (support.dtype, support.shape)
    _, m = check_nodata("keep", min_support)
    if support_u8 is not None:
        assert support_u8.is_cuda and support_u8.dtype == torch.uint8 and support_u8.is_contiguous() and \
            tuple(support_u8.shape) == (H, W), (support_u8.dtype, support_u8.shape)
    hip.check(hip.lib().ssr_scene_apply_nodata(_ptr(mosaic), Ho, Wo, C, _ptr(support), m,
                                               None if support_u8 is None else _ptr(support_u8), hip.stream_ptr()),
              "ssr_scene_apply_nodata")


def _blend_add(src: torch.Tensor, origins: torch.Tensor, tf: Optional[torch.Tensor], C: int, window: torch.Tensor, acc: torch.Tensor,
               nonfinite: torch.Tensor, dtype: Optional[int]):
    """the body of the two blend-adds: `ssr_scene_blend_add_tf` with transform ids, else `ssr_scene_blend_add`"""
    from . import hip
    B = origins.shape[0]
    _check_origins(origins)
    _check_acc(acc, C)
    assert tuple(src.shape[:3]) == (B, SR_CHUNK, SR_CHUNK) and src.shape[3] >= C, src.shape
    assert window.is_cuda and window.dtype == torch.int32 and window.is_contiguous() and tuple(window.shape) == (SR_CHUNK,)
    assert nonfinite.dtype == torch.int32 and nonfinite.is_cuda
    if dtype is None:
        dtype = hip.dtype_code(src.dtype)
    tail = (B, C, _ptr(window), _ptr(acc), acc.shape[0], acc.shape[1], _ptr(nonfinite), hip.stream_ptr())
    if tf is not None:
        _check_tf(tf, B)
        hip.check(hip.lib().ssr_scene_blend_add_tf(hip.view(src), dtype, _ptr(origins), _ptr(tf), *tail), "ssr_scene_blend_add_tf")
    else:
        hip.check(hip.lib().ssr_scene_blend_add(hip.view(src), dtype, _ptr(origins), *tail), "ssr_scene_blend_add")


def scene_blend_add(src: torch.Tensor, origins: torch.Tensor, C: int, window: torch.Tensor, acc: torch.Tensor,
                    nonfinite: torch.Tensor, dtype: Optional[int] = None):
    """src, an NHWC generator output [B, 128, 128, >= C], in 16-bit fixed point times the window weights (int32 [128], device) is
    added to acc (int32 storage [Ho, Wo, C] on the device, read as uint32) at 4 x the origins; adds the number of non-finite
    samples to the int32 device counter"""
    _blend_add(src, origins, None, C, window, acc, nonfinite, dtype)


def scene_blend_add_tf(src: torch.Tensor, origins: torch.Tensor, tf: torch.Tensor, C: int, window: torch.Tensor, acc: torch.Tensor,
                       nonfinite: torch.Tensor, dtype: Optional[int] = None):
    """`scene_blend_add` of `ensemble_inverse(src[b], tf[b])` (tf int32 [B], device) in 13-bit fixed point (`ENSEMBLE_ONE`): the
    eight rows of a chunk add up in acc, which `scene_blend_finish_scaled` divides by 8 x 8191 x the weight sums"""
    assert tf is not None
    _blend_add(src, origins, tf, C, window, acc, nonfinite, dtype)


def _blend_finish(acc: torch.Tensor, Sy: torch.Tensor, Sx: torch.Tensor, mosaic: torch.Tensor, scale: Optional[int]):
    """the body of the two finishes: `ssr_scene_blend_finish_scaled` with a scale, else `ssr_scene_blend_finish`"""
    from . import hip
    Ho, Wo, C = acc.shape
    _check_acc(acc, C)
    assert mosaic.is_cuda and mosaic.dtype == torch.uint8 and mosaic.is_contiguous() and tuple(mosaic.shape) == (Ho, Wo, C)
    for S, L in ((Sy, Ho), (Sx, Wo)):
        assert S.is_cuda and S.dtype == torch.int32 and S.is_contiguous() and tuple(S.shape) == (L,)
    tail = (_ptr(mosaic), Ho, Wo, hip.stream_ptr())
    if scale is not None:
        assert 1 <= scale < 1 << 31, scale
        hip.check(hip.lib().ssr_scene_blend_finish_scaled(_ptr(acc), _ptr(Sy), _ptr(Sx), C, scale, *tail), "ssr_scene_blend_finish_scaled")
    else:
        hip.check(hip.lib().ssr_scene_blend_finish(_ptr(acc), _ptr(Sy), _ptr(Sx), C, *tail), "ssr_scene_blend_finish")


def scene_blend_finish(acc: torch.Tensor, Sy: torch.Tensor, Sx: torch.Tensor, mosaic: torch.Tensor):
    """acc [Ho, Wo, C] over the weight sums Sy (int32 [Ho]) and Sx (int32 [Wo]) -> mosaic, uint8 [Ho, Wo, C], truncating"""
    _blend_finish(acc, Sy, Sx, mosaic, None)


def scene_blend_finish_scaled(acc: torch.Tensor, Sy: torch.Tensor, Sx: torch.Tensor, mosaic: torch.Tensor, scale: int):
    """`scene_blend_finish` with the denominator's scale given: mosaic = acc * 255 // (Sy Sx scale); ENSEMBLE * ENSEMBLE_ONE under
    the self-ensemble"""
    _blend_finish(acc, Sy, Sx, mosaic, int(scale))


def merc_to_utm_coords(window, georef, device=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`s2_reproject.source_coords` on the device (`ssr_merc_to_utm_coords`): window (a Window or a window mapping) and georef (a
    Georef or its mapping) -> int32 [h, w, 2] on the device, (U, V) of every pixel centre in 16.16 fixed point, INT32_MIN in both
    words outside the raster.  The same refusals as the statement, on the host, before the launch."""
    from . import hip, s2_reproject as S
    win, g = S.parse_window(window), S.check_georef(georef)
    if out is None:
        out = torch.empty(win.h, win.w, 2, dtype=torch.int32, device=torch.device("cuda") if device is None else device)
    assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (win.h, win.w, 2), (out.dtype, out.shape)
    hip.check(hip.lib().ssr_merc_to_utm_coords(win.px0, win.py0, win.w, win.h, g.epsg, g.ulx, g.uly, g.xdim, g.ydim, g.rows, g.cols,
                                               _ptr(out), hip.stream_ptr()), "ssr_merc_to_utm_coords")
    return out


def scene_warp(src: torch.Tensor, coords: torch.Tensor, nodata: str = "blend", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`s2_reproject.warp_bilinear` on the device (`ssr_scene_warp_bilinear`): src uint8 [T, Hs, Ws, C] (C = 1 or 3, any address) and
    coords int32 [h, w, 2] (`merc_to_utm_coords`), both on the device -> uint8 [T, h, w, C] on the device; every frame reads the one
    coordinate array.  nodata: "blend" or "propagate", as the statement."""
    from . import hip, s2_reproject as S
    if nodata not in S.NODATA_MODES:
        raise ValueError(f"reproject_nodata = {nodata!r}: one of {', '.join(S.NODATA_MODES)}")
    assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 4 and src.shape[3] in (1, 3) \
        and src.numel() > 0, (src.dtype, src.shape)
    assert coords.is_cuda and coords.dtype == torch.int32 and coords.is_contiguous() and coords.dim() == 3 and coords.shape[2] == 2 \
        and coords.numel() > 0, (coords.dtype, coords.shape)
    T, Hs, Ws, C = src.shape
    h, w = coords.shape[:2]
    if max(h, w) > S.MAX_WINDOW or max(Hs, Ws) > S.MAX_RASTER:
        raise ValueError(f"a warp of a {Hs} x {Ws} source into {h} x {w} pixels: at most {S.MAX_RASTER} and {S.MAX_WINDOW} per side")
    if out is None:
        out = torch.empty(T, h, w, C, dtype=torch.uint8, device=src.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (T, h, w, C), (out.dtype, out.shape)
    hip.check(hip.lib().ssr_scene_warp_bilinear(_ptr(src), T, Hs, Ws, C, _ptr(coords), h, w, S.NODATA_MODES.index(nodata), _ptr(out),
                                                hip.stream_ptr()), "ssr_scene_warp_bilinear")
    return out


def reproject_scene(rasters, georefs, window, nodata: str = "blend", device=None) -> torch.Tensor:
    """Raw Sentinel-2 frames onto the model's grid, on the device: rasters, T uint8 arrays [Hs, Ws, 3] (numpy; each frame its own
    size), georefs, their T georeferences (`s2_reproject.Georef` or its mapping: UTM, `ulx` / `uly` the outer corner of the array's
    first pixel), window (a window mapping, `s2_reproject.parse_window`) -> uint8 [T, h, w, 3] on the device, what
    `super_resolve_scene(_blended)` take as `frames`.  `s2_reproject.py` states the result (`source_coords`, `warp_bilinear`); it is
    not GDAL's.
    Of every raster only the rectangle the window needs (`source_crop`, padded by 2 pixels) is uploaded, with its own georeference;
    frames whose crops share a georeference and a size are stacked and warped by ONE launch from ONE coordinate array; a frame the
    window misses altogether stays 0.  nodata: "blend" (plain bilinear) or "propagate" (a zero sample with non-zero weight makes the
    pixel NODATA)."""
    from . import s2_reproject as S
    win = S.parse_window(window)
    if nodata not in S.NODATA_MODES:
        raise ValueError(f"reproject_nodata = {nodata!r}: one of {', '.join(S.NODATA_MODES)}")
    rasters, georefs = list(rasters), [S.check_georef(g) for g in georefs]
    if not rasters or len(rasters) != len(georefs):
        raise ValueError(f"{len(rasters)} rasters with {len(georefs)} georeferences")
    crops: List[Optional[np.ndarray]] = []
    crop_georefs: List[Optional[S.Georef]] = []
    for t, (a, g) in enumerate(zip(rasters, georefs)):
        a = np.asarray(a)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[:2] != (g.rows, g.cols):
            raise ValueError(f"raster {t}: a uint8 array [{g.rows}, {g.cols}, 3] by its georeference, not {a.dtype} {tuple(a.shape)}")
        box = S.source_crop(win, g)
        crops.append(None if box is None else a[box[1]:box[3], box[0]:box[2]])
        crop_georefs.append(None if box is None else S.crop_georef(g, box))
    return _warp_crops(crops, crop_georefs, win, nodata, torch.device("cuda") if device is None else device)


def _warp_crops(crops, crop_georefs, win, nodata: str, dev) -> torch.Tensor:
    """the device half of `reproject_scene`: the frames' crops (uint8 [Hc, Wc, 3] on the host, or None for a frame the window
    misses) with their own georeferences -> uint8 [T, h, w, 3] on the device.  Frames that share a georeference are stacked,
    uploaded once and warped by one launch from one coordinate array."""
    groups: Dict = {}
    for t, g in enumerate(crop_georefs):
        if g is not None:
            groups.setdefault(g, []).append(t)
    out = torch.zeros(len(crops), win.h, win.w, 3, dtype=torch.uint8, device=dev)
    for g, ts in groups.items():
        src = torch.from_numpy(np.stack([crops[t] for t in ts])).to(dev)
        coords = merc_to_utm_coords(win, g, dev)
        if ts == list(range(ts[0], ts[0] + len(ts))):
            scene_warp(src, coords, nodata, out[ts[0]:ts[0] + len(ts)])          # a run of frames: straight into its place
        else:
            out[torch.tensor(ts, device=dev)] = scene_warp(src, coords, nodata)
    return out


class _Pending:
    """a scene whose launches are queued: the pinned host buffer its mosaic and counter (under `nodata: keep` the support map
    behind them) are being copied to, and the event behind that copy"""

    def __init__(self, host, event, shape, compute_dtype, chunks, support_off: Optional[int] = None):
        self.host, self.event, self.shape, self.compute_dtype, self.chunks = host, event, shape, compute_dtype, chunks
        self.support_off = support_off          # where the uint8 [H, W] support map starts in the buffer; None under `fill`

    def result(self, where: str = "") -> np.ndarray:
        """waits for the download; raises FloatingPointError if an output sample was NaN / Inf (before any pixel is handed out)"""
        from .metrics import nonfinite_error, split_checked
        self.event.synchronize()
        img, bad = split_checked(self.host, self.shape)
        if bad:
            raise nonfinite_error(bad, self.compute_dtype, where)
        return img.numpy()

    def support(self) -> np.ndarray:
        """after `result()`, under `nodata: keep`: uint8 [H, W], min(support, 255)"""
        assert self.support_off is not None, "a support map comes back under nodata = 'keep' only"
        self.event.synchronize()
        H, W = self.shape[0] // SCALE, self.shape[1] // SCALE
        return self.host[self.support_off:self.support_off + H * W].view(H, W).numpy()


def _check_bands(model, frames, bands, n: int):
    """the refusals of a `bands` argument, before anything is uploaded: uint8 [K, T, H, W] with the frames' T, H, W and a generator
    of n (3 + K) channels"""
    if not isinstance(bands, torch.Tensor):
        bands = np.asarray(bands)
    u8 = torch.uint8 if isinstance(bands, torch.Tensor) else np.uint8
    if bands.dtype != u8 or len(bands.shape) != 4 or bands.shape[0] < 1:
        raise ValueError(f"bands are a uint8 array [K, T, H, W], not {bands.dtype} {tuple(bands.shape)}")
    if len(frames.shape) == 4 and tuple(bands.shape[1:]) != tuple(frames.shape[:3]):
        raise ValueError(f"bands of T, H, W = {tuple(bands.shape[1:])} beside frames of T, H, W = {tuple(frames.shape[:3])}")
    K, C_in = int(bands.shape[0]), model.kwargs["num_in_ch"]
    if C_in != n * (3 + K):
        raise ValueError(f"n_lr_images = {n} with {K} extra band(s) gives {n * (3 + K)} input channels, the generator takes {C_in}")
    return bands


def _upload_scene(model, frames, n: int, any_size: bool = False, bands=None) -> Tuple[torch.Tensor, int, Optional[torch.Tensor]]:
    """the checks of the scene and of the generator's channels, the upload: (uint8 [T, H, W, 3] on the model's device, num_out_ch,
    the bands as uint8 [K, T, H, W] on that device or None)"""
    dev = next(model.parameters()).device
    if bands is not None:
        bands = _check_bands(model, frames if isinstance(frames, torch.Tensor) else np.asarray(frames), bands, n)
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError(f"a scene is a uint8 array [T, H, W, 3], not {frames.dtype} {tuple(frames.shape)}")
        check_scene_size(frames.shape[1], frames.shape[2], any_size)
        scene = frames.to(dev, non_blocking=True).contiguous()
    else:
        arr = np.asarray(frames)
        if arr.ndim != 4:
            raise ValueError(f"a scene is a uint8 array [T, H, W, 3], not {arr.dtype} {tuple(arr.shape)}")
        arr = parse_scene(arr, any_size=any_size)
        arr = np.ascontiguousarray(arr) if arr.flags.writeable else np.array(arr)      # (a read-only mapping of a .npy file: copy)
        scene = torch.from_numpy(arr).to(dev, non_blocking=True)
    C_in, C_out = model.kwargs["num_in_ch"], model.kwargs["num_out_ch"]
    if bands is None:
        if C_in != 3 * n:
            raise ValueError(f"n_lr_images = {n} gives {3 * n} input channels, the generator takes {C_in}")
        return scene, C_out, None
    if not isinstance(bands, torch.Tensor):
        bands = torch.from_numpy(np.ascontiguousarray(bands) if bands.flags.writeable else np.array(bands))
    return scene, C_out, bands.to(dev, non_blocking=True).contiguous()


def _download_buffer(dev, Ho: int, Wo: int, C_out: int, keep: bool):
    """the one buffer a scene downloads: the mosaic and, behind it, the counter (zeroed here); under `nodata: keep` the counter's 16
    bytes are followed by the uint8 [H, W] support map.  -> (buffer, mosaic view, counter view, support view or None, its offset or None)"""
    nb = Ho * Wo * C_out
    off = -(-nb // 16) * 16
    n_sup = (Ho // SCALE) * (Wo // SCALE) if keep else 0
    buf = torch.empty(off + (16 + n_sup if keep else 4), dtype=torch.uint8, device=dev)
    counter = buf[off:off + 4].view(torch.int32)
    counter.zero_()
    mosaic = buf[:nb].view(Ho, Wo, C_out)
    if not keep:
        return buf, mosaic, counter, None, None
    return buf, mosaic, counter, buf[off + 16:].view(Ho // SCALE, Wo // SCALE), off + 16


def _frames_T(frames) -> Optional[int]:
    """the frame count of a scene argument before it is parsed (None for what `_upload_scene` refuses anyway)"""
    shape = getattr(frames, "shape", None)
    if shape is None:
        shape = np.asarray(frames).shape
    return int(shape[0]) if len(shape) == 4 else None


def _enqueue_scene(model, frames, n_lr_images: int, batch: int, host: Optional[torch.Tensor] = None, bands=None,
                   frame_select: str = "random", nodata: str = "fill", min_support: int = 1, self_ensemble: bool = False,
                   blended: bool = False, overlap: int = 0) -> _Pending:
    """Everything a scene queues, without waiting for it: upload, frame choice, every batch of generator rows through gather ->
    generator -> write-out, and the one download of mosaic + counter.
    The frame choice: under frame_select "random" a zero scan and the one host round trip (chunks x T flags down, chunks x n ids
    up); under "clearest" keys -> rank on the current stream, and nothing comes back to the host before the mosaic does.
    The write-out is the one difference between the two paths.  The grid path (not blended: H and W multiples of 32, the chunks at
    (32 i, 32 j) in row-major order) gathers with `scene_gather` (with bands: `scene_gather_bands` at those origins) and writes
    straight into the mosaic with `scene_scatter_u8`; it allocates no accumulator.  The accumulator path (blended: any size >= 32 x
    32, chunks that overlap by `overlap`) gathers at the origins, adds into a zeroed uint32 accumulator of this scene's own
    (`scene_blend_add`) and divides by the weight sums (`scene_blend_finish`).
    nodata "keep": a zeroed support map, `scene_support_add` beside the gather, once per chunk, `scene_apply_nodata` behind the last
    write-out, and the support map behind the counter in the same download; nothing comes back earlier than without it.
    self_ensemble: always the accumulator path - not blended it is overlap 0, the same chunks in the same order and so the same
    frame choice, under the grid path's refusal of sizes that are no multiples of 32.  The generator's rows are the (chunk, tf)
    pairs, chunk-major with tf 0 .. 7 inside a chunk, and `batch` slices THAT list: gather_tf -> generator -> blend_add_tf per
    slice, then `scene_blend_finish_scaled`.  The frames are chosen once per chunk as without it, and `scene_support_add` runs
    beside the slice that holds the chunk's tf 0 row."""
    self_ensemble = check_self_ensemble(self_ensemble)          # (the refusals, in this order, before anything is uploaded)
    if getattr(model, "scale", SCALE) != SCALE:
        raise NotImplementedError(f"scene inference runs scale {SCALE} generators only (scale = {model.scale})")
    n, batch = int(n_lr_images), int(batch)
    if batch < 1:
        raise ValueError(f"batch = {batch}")
    accumulate = blended or self_ensemble
    if not blended:
        overlap = 0
    if accumulate:
        window = blend_window(overlap)
    check_frame_select(frame_select, _frames_T(frames), n)
    nodata, min_support = check_nodata(nodata, min_support)
    keep = nodata == "keep"
    scene, C_out, bands = _upload_scene(model, frames, n, any_size=blended, bands=bands)
    dev = scene.device
    T, H, W = scene.shape[:3]
    grid = scene_chunk_grid(H, W, overlap)          # on the grid path (32 i, 32 j) in row-major order
    n_chunks = grid.shape[0]
    origins = None
    if accumulate or bands is not None or keep or frame_select == "clearest":
        origins = torch.from_numpy(grid).to(dev, non_blocking=True)
    if accumulate:
        window = torch.from_numpy(window).to(dev, non_blocking=True)
        Sy = torch.from_numpy(blend_weight_sums(H, overlap)).to(dev, non_blocking=True)
        Sx = torch.from_numpy(blend_weight_sums(W, overlap)).to(dev, non_blocking=True)
    if frame_select == "clearest":
        frame_ids = scene_rank_frames(scene_frame_keys(scene, origins), n)
    else:
        has_zero = (scene_zero_scan_at(scene, origins) if accumulate else scene_zero_scan(scene)).cpu().numpy()
        frame_ids = torch.from_numpy(select_scene_frames(has_zero, n)).to(dev, non_blocking=True)
    Ho, Wo = SCALE * H, SCALE * W
    buf, mosaic, counter, support_u8, support_off = _download_buffer(dev, Ho, Wo, C_out, keep)      # one download
    support = torch.zeros(H, W, dtype=torch.int32, device=dev) if keep else None
    if accumulate:
        acc = torch.zeros(Ho, Wo, C_out, dtype=torch.int32, device=dev)  # 4 bytes per output sample, this scene's own
    else:
        chunk_ids = torch.arange(n_chunks, dtype=torch.int32, device=dev)
    per = ENSEMBLE if self_ensemble else 1          # generator rows per chunk
    row_org, row_ids, row_tf = origins, frame_ids, None
    if self_ensemble:                               # the rows: (chunk, tf), chunk-major
        row_org, row_ids = origins.repeat_interleave(ENSEMBLE, dim=0), frame_ids.repeat_interleave(ENSEMBLE, dim=0)
        row_tf = torch.arange(ENSEMBLE, dtype=torch.int32, device=dev).repeat(n_chunks)
    with torch.no_grad():
        for r0 in range(0, per * n_chunks, batch):
            r1 = min(r0 + batch, per * n_chunks)
            plan = model.plan_for_inference(r1 - r0, CHUNK, CHUNK)
            tf = None if row_tf is None else row_tf[r0:r1]
            if accumulate or bands is not None:
                _gather_at(scene, bands, row_org[r0:r1], row_ids[r0:r1], tf, plan.xin, plan.dt)
            else:
                scene_gather(scene, chunk_ids[r0:r1], row_ids[r0:r1], plan.xin, plan.dt)
            c0, c1 = -(-r0 // per), -(-r1 // per)   # the chunks whose first row lies in this slice
            if keep and c1 > c0:
                scene_support_add(scene, origins[c0:c1], frame_ids[c0:c1], support)
            model.run_forward(plan)
            if accumulate:
                _blend_add(plan.out, row_org[r0:r1], tf, C_out, window, acc, counter, plan.dt)
            else:
                scene_scatter_u8(plan.out, chunk_ids[r0:r1], C_out, mosaic, counter, plan.dt)
        if accumulate:
            _blend_finish(acc, Sy, Sx, mosaic, ENSEMBLE * ENSEMBLE_ONE if self_ensemble else None)
            del acc
        if keep:
            scene_apply_nodata(mosaic, support, min_support, support_u8)
    if host is None or host.numel() != buf.numel():
        host = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(buf, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return _Pending(host, ev, (Ho, Wo, C_out), getattr(model, "compute_dtype", None), n_chunks, support_off)


def _check_return_support(nodata, min_support, return_support) -> None:
    """the refusals of the public entry points' NODATA arguments, before anything is uploaded"""
    nodata, _ = check_nodata(nodata, min_support)
    if return_support and nodata != "keep":
        raise ValueError(f"return_support: a support map comes back under nodata = 'keep' only (nodata = {nodata!r})")


def _finish(pending: _Pending, return_support: bool):
    mosaic = pending.result()
    return (mosaic, pending.support()) if return_support else mosaic


def super_resolve_scene_blended(model, frames, n_lr_images: int, overlap: int = 8, batch: int = 64, bands=None,
                                frame_select: str = "random", nodata: str = "fill", min_support: int = 1,
                                return_support: bool = False, self_ensemble: bool = False):
    """frames: uint8 [T, H, W, 3] (numpy array or CUDA tensor), H and W ANY values >= 32 -> uint8 [4H, 4W, 3].  The scene is cut into
    32 x 32 chunks that overlap their neighbours by `overlap` pixels (0 .. 16; `scene_chunk_origins`: the last chunk of an axis ends
    at the scene's edge), every chunk is super-resolved from `n_lr_images` of its frames (select_scene_frames over the chunks in
    row-major order) and the outputs are cross-faded where they overlap (`blend_window`), in integer arithmetic on the device: the
    bytes do not depend on the batch size or the order of the chunks.
    The accumulator holds 4 bytes per output sample (48 H W bytes: 50 MB for 512 x 512, 23 GB for a whole 10980 x 10980
    acquisition) and is allocated per scene, next to the scene itself and the 12 H W bytes of the mosaic.
    Refusals as `super_resolve_scene`: scale 4 generators only, n_lr_images against the generator's channels, FloatingPointError
    (metrics.nonfinite_error) if any output sample is NaN / Inf.  `bands`, `frame_select`, `nodata`, `min_support` and
    `return_support` as `super_resolve_scene`; here up to 3 chunks per axis cover a pixel, so support <= 9 n_lr_images.
    self_ensemble=True (a bool, ValueError otherwise, before anything is uploaded) is BasicSR's `val.self_ensemble`
    (SRModel.test_selfensemble) over chunks: every chunk goes through the generator under the eight flips and transposes of the
    square (`ensemble_transform`, tf 0 .. 7), the eight outputs are turned back (`ensemble_inverse`) and averaged.  The transform set
    is BasicSR's; the averaging is this project's integer blend, not a float mean, so the bytes are not BasicSR's: every output in
    13-bit fixed point (`ENSEMBLE_ONE`), times the blend window, into the same accumulator, and
    mosaic = acc * 255 // (8 * Sy * Sx * 8191).  The generator's rows are the (chunk, tf) pairs in chunk-major order and `batch`
    slices that list, so a scene costs eight times the generator launches' rows; integer sums keep the bytes independent of
    `batch`.  Frames are chosen once per chunk exactly as without it (all eight transforms of a chunk use them, `random` is
    consumed once per chunk), support and `nodata` are what they are without it, and the non-finite count covers all eight
    outputs.  With `frame_select="clearest"` the mosaic of a flipped or transposed scene is the flipped or transposed mosaic, byte
    for byte, when the chunk origins are symmetric about the centre."""
    _check_return_support(nodata, min_support, return_support)
    return _finish(_enqueue_scene(model, frames, n_lr_images, batch, bands=bands, frame_select=frame_select, nodata=nodata,
                                  min_support=min_support, self_ensemble=check_self_ensemble(self_ensemble), blended=True,
                                  overlap=overlap), return_support)


def super_resolve_scene(model, frames, n_lr_images: int, batch: int = 64, bands=None, frame_select: str = "random",
                        nodata: str = "fill", min_support: int = 1, return_support: bool = False, self_ensemble: bool = False):
    """frames: uint8 [T, H, W, 3] (numpy array or CUDA tensor), H and W multiples of 32 (ValueError otherwise) -> uint8
    [4H, 4W, 3]: every 32 x 32 chunk super-resolved on its own from `n_lr_images` of its frames (select_scene_frames) and placed
    at rows 128 i, columns 128 j.  Raises FloatingPointError (metrics.nonfinite_error) if any output sample is NaN / Inf.
    bands: uint8 [K, T, H, W] (numpy array or CUDA tensor), the K extra Sentinel-2 bands of a multi-band generator, which then takes
    n_lr_images * (3 + K) channels - per chosen frame the TCI, then the bands in their order, what `S2NAIPDataset` with `s2_bands`
    feeds it in training; the frames are chosen on the TCI alone.  ValueError, before anything is uploaded, for bands of another
    rank, dtype or T, H, W than the frames' and for a generator of another channel count.
    frame_select: "random" (the default) is the reference's rule, `select_scene_frames`, which consumes the `random` module;
    "clearest" is this project's own, deterministic policy, computed on the device (`rank_scene_frames` states it): per chunk the
    n_lr_images frames with the fewest NODATA pixels, then the fewest saturated ones, then the lower index, best frame first.  Its
    chosen set is always one the reference's rule could have drawn (all clean frames if there are fewer than n, else n clean ones),
    nothing is copied to the host or waited for between the upload and the download of the mosaic, and `random` is not consumed.
    ValueError, before anything is uploaded, for another value, and under "clearest" for fewer than n_lr_images frames or more than
    1024.
    nodata: "fill" (the default) runs the generator on ESA's NODATA (the value 0 of the TCI) and writes whatever it makes of it,
    as the reference does.  "keep" is this project's own policy (the reference has no counterpart file): NODATA in, NODATA out.  A
    low-resolution pixel of a frame HAS DATA if none of its three TCI samples is 0 (bands take no part); support[y, x] is the number
    of pairs (chunk that covers (y, x), chosen frame slot of that chunk) whose TCI pixel at (y, x) has data - what went into the
    generator, here at most n_lr_images (`scene_support` states it).  Every sample of the 4 x 4 output block of a pixel with
    support < min_support (an integer >= 1) becomes 0, every other sample max(1, sample): 0 stays reserved for NODATA
    (`apply_nodata`).  Computed on the device, without a further round trip; a NaN / Inf under a masked pixel still raises.
    return_support=True returns (mosaic, support_u8) with support_u8 = min(support, 255), uint8 [H, W].  ValueError, before anything
    is uploaded, for another value of nodata, a min_support that is not an integer >= 1 or differs from 1 under "fill", and
    return_support without "keep".
    self_ensemble=True: as `super_resolve_scene_blended(..., overlap=0, self_ensemble=True)` - the eight flips and transposes of
    every chunk through the generator, turned back and averaged by the integer blend at 13 fractional bits - with this function's
    refusal of sizes that are no multiples of 32.  A bool; ValueError otherwise, before anything is uploaded."""
    _check_return_support(nodata, min_support, return_support)
    return _finish(_enqueue_scene(model, frames, n_lr_images, batch, bands=bands, frame_select=frame_select, nodata=nodata,
                                  min_support=min_support, self_ensemble=check_self_ensemble(self_ensemble)), return_support)


# ------------------------------------------------------------------------------------------------ driver
def run_infer_scene(opt: Dict, model=None, rank: int = 0, world: int = 1, device=None) -> Dict:
    from . import png_io
    from .infer_grid import load_generator
    data_dir, save_path, n_lr_images = opt["data_dir"], opt["save_path"], int(opt["n_lr_images"])
    batch, scene_hw = int(opt.get("batch", 64)), opt.get("scene_hw")
    overlap = opt.get("overlap")                    # absent: every chunk on its own (the reference's mosaic); 0 .. 16: blended
    blended = overlap is not None
    if blended:
        scene_chunk_origins(CHUNK, overlap)
    frame_select = check_frame_select(opt.get("frame_select", "random"))      # absent: random, the reference's rule
    nodata, min_support = check_nodata(opt.get("nodata", "fill"), opt.get("nodata_min_support", 1))      # absent: fill, as ever
    keep = nodata == "keep"
    self_ensemble = check_self_ensemble(opt.get("self_ensemble", False))      # absent: false, the launches of the paths above
    source = check_source(opt.get("source"), opt.get("s2_bands"))             # absent: scenes on the grid, nothing new runs
    if source is not None:
        from . import s2_reproject as S2
        s2_window = S2.parse_window(opt.get("window"))
        reproject_nodata = opt.get("reproject_nodata", "blend")
        if reproject_nodata not in S2.NODATA_MODES:
            raise ValueError(f"reproject_nodata = {reproject_nodata!r}: one of {', '.join(S2.NODATA_MODES)}")
    if device is None:
        device = torch.device("cuda")
    if model is None:
        model = load_generator(opt, device)
    s2_bands = opt.get("s2_bands")                  # absent: scene files NAME.png / NAME.npy; given: scene directories NAME/<band>.png
    K = 0 if s2_bands is None else len(order_s2_bands(s2_bands)) - 1
    if source is not None:
        scenes = list_product_scenes(data_dir)
        png_io.check_raster_decoders([p for _, products in scenes for p in products])      # at start-up: names what Pillow lacks
    else:
        scenes = list_scenes(data_dir) if s2_bands is None else list_band_scenes(data_dir, s2_bands)
    if rank == 0:
        print("Running inference on ", len(scenes), " scenes.")
    mine = scenes_of_rank(scenes, rank, world)
    # worker budget as infer_grid's: the cores this process may really use, shared by the ranks of the node, one left to the driver
    workers = int(opt.get("io_workers", max(1, min(16, png_io.host_cores() // max(1, world) - 1))))
    t_start = time.perf_counter()
    chunks = 0
    import contextlib
    with contextlib.ExitStack() as stack:
        open_blocks: List = []
        stack.callback(lambda: [b.close() for b in list(open_blocks)])      # registered first: runs after the last task has ended
        pool = stack.enter_context(png_io.shared_pool(workers))
        sdir = None

        def block(nbytes, tag):
            nonlocal sdir
            if sdir is None:
                sdir = png_io.shm_dir(4 * nbytes)
            blk = png_io.ShmBlock(nbytes, sdir, f"r{rank}_{tag}")
            open_blocks.append(blk)
            return blk

        def release(blk):
            blk.close()
            if blk in open_blocks:
                open_blocks.remove(blk)

        def start_read(k):
            """scene k's pixels on their way to host memory: a PNG is decoded by a worker into a one-shot block, a .npy is mapped"""
            if source is not None:
                return start_read_products(*mine[k])
            if s2_bands is not None:
                return start_read_bands(*mine[k])
            name, path = mine[k]
            if path.lower().endswith(".npy"):
                return name, None, None, np.load(path, mmap_mode="r")
            shape = _png_shape(path)
            blk = block(int(np.prod(shape)), "scene")
            return name, blk, [pool.submit("read_into", [path], blk.path, blk.nbytes, [0], blk.nbytes, True)], shape

        def start_read_bands(name, tci, band_paths):
            """a scene directory: tci.png and every band file that exists are decoded side by side into one block - the TCI first,
            behind it the K planes [K][T*H][W]; the plane of a missing band stays zero (the block is new)"""
            rows, W = band_scene_shape(tci, band_paths)          # (refuses a band file of another size or mode by name)
            npix = rows * W
            blk = block((3 + K) * npix, "scene")
            futs = [pool.submit("read_into", [tci], blk.path, blk.nbytes, [0], 3 * npix, True)]
            futs += [pool.submit("read_gray_into", p, blk.path, blk.nbytes, (3 + kb) * npix, (rows, W), True)
                     for kb, p in enumerate(band_paths) if p is not None]
            return name, blk, futs, (rows, W, 3)

        def start_read_products(name, products):
            """a scene of raw products: per product the georeference (MTD_TL.xml or the sidecar), the source rectangle the window
            needs, and a worker that decodes the raster and writes that rectangle into the scene's block"""
            found = [S2.find_product(p) for p in products]
            plan, off = [], 0
            for f, g in found:
                if png_io.raster_size(f) != (g.rows, g.cols):
                    raise ValueError(f"{f}: {png_io.raster_size(f)} pixels, its georeference says {(g.rows, g.cols)}")
                box = S2.source_crop(s2_window, g)
                plan.append(None if box is None else (f, box, S2.crop_georef(g, box), off))
                off += 0 if box is None else 3 * (box[2] - box[0]) * (box[3] - box[1])
            blk = block(off, "scene") if off else None
            futs = [pool.submit("read_crop_into", f, box, blk.path, blk.nbytes, o, True) for f, box, _, o in filter(None, plan)]
            return name, blk, futs, plan

        def finish_read_products(rd):
            """the crops are in the block: upload, coordinates, warp - the scene as a device tensor [T, h, w, 3]"""
            name, blk, futs, plan = rd
            shapes = iter([f.result() for f in futs])
            crops = []
            for p in plan:
                sh = None if p is None else next(shapes)
                crops.append(None if p is None else blk.buf[p[3]:p[3] + int(np.prod(sh))].reshape(sh))
            frames = _warp_crops(crops, [None if p is None else p[2] for p in plan], s2_window, reproject_nodata, device)
            return name, blk, frames, None

        def finish_read(rd) -> Tuple[str, object, np.ndarray, Optional[np.ndarray]]:
            if source is not None:
                return finish_read_products(rd)
            name, blk, futs, what = rd
            if blk is None:
                return name, None, parse_scene(np.asarray(what), scene_hw, blended), None
            got = [f.result() for f in futs][0][0]
            arr = got if isinstance(got, np.ndarray) else blk.buf[:int(np.prod(got))].reshape(got)
            frames = parse_scene(arr, scene_hw, blended)
            if not K:
                return name, blk, frames, None
            return name, blk, frames, blk.buf[frames.size:].reshape((K,) + frames.shape[:3])

        def submit_save(arr: np.ndarray, path: str):
            """one image to an encoder through a block of its own (closed and unlinked as soon as the file is written)"""
            blk = block(arr.nbytes, "mosaic")
            blk.buf[:] = arr.reshape(-1)
            f = pool.submit("save_from", blk.path, blk.nbytes, [(0, tuple(arr.shape), path)], True)
            f.add_done_callback(lambda _f, b=blk: release(b))
            return f

        # software pipeline over the scenes: scene k + 1 is being decoded and scene k - 1 encoded while the device runs scene k
        saves = []
        stack.callback(lambda: [f.exception() for f in saves])     # runs first, also on an error: earlier scenes' files are whole
        hosts = [None, None]
        reading = start_read(0) if mine else None
        prev = None                                   # (name, first frame, pending, block) of the scene the device is running
        for k in range(len(mine) + 1):
            cur = None
            if k < len(mine):
                name, blk, frames, bands = finish_read(reading)
                reading = start_read(k + 1) if k + 1 < len(mine) else None
                # the reprojected frame 0 comes back BEFORE the scene's launches are queued: the copy waits for the warp alone
                first = frames[0].cpu().numpy() if source is not None else None
                pending = _enqueue_scene(model, frames, n_lr_images, batch, hosts[k & 1], bands=bands, frame_select=frame_select,
                                         nodata=nodata, min_support=min_support, self_ensemble=self_ensemble, blended=blended,
                                         overlap=overlap)
                hosts[k & 1] = pending.host
                if first is None:
                    first = np.array(frames[0])
                del frames, bands
                if frame_select == "random" or source is not None:      # (source: the crops were uploaded before frame 0 came back)
                    if blk is not None:
                        release(blk)                                # (the upload has been waited for: the flags came back)
                    blk = None
                cur = (name, first, pending, blk)                   # clearest: nothing came back yet, the block lives until the mosaic does
            if prev is not None:
                pname, first, ppend, pblk = prev
                sr = ppend.result(f" in scene {pname}")             # raises before any file of the scene is written
                if pblk is not None:
                    release(pblk)
                saves.append(submit_save(sr, os.path.join(save_path, pname, "stitched_sr.png")))
                saves.append(submit_save(first, os.path.join(save_path, pname, "stitched_s2.png")))
                if keep:
                    saves.append(submit_save(ppend.support(), os.path.join(save_path, pname, "stitched_support.png")))
                if source is not None:                              # what places the two mosaics in a GIS
                    import json
                    for stem, scale in (("stitched_sr", SCALE), ("stitched_s2", 1)):
                        os.makedirs(os.path.join(save_path, pname), exist_ok=True)
                        with open(os.path.join(save_path, pname, stem + ".json"), "w") as f:
                            json.dump(S2.window_georef(s2_window, scale), f, indent=1)
                chunks += ppend.chunks
            prev = cur
        for f in saves:
            f.result()
    res = {"scenes": len(mine), "chunks": chunks, "seconds": round(time.perf_counter() - t_start, 3), "io_workers": workers,
           "frame_select": frame_select}
    if keep:
        res.update(nodata=nodata, nodata_min_support=min_support)
    if self_ensemble:
        res.update(self_ensemble=True)
    if source is not None:
        res.update(source=source, window_pixels=list(s2_window), reproject_nodata=reproject_nodata)
    return res


def main():
    import yaml
    parser = argparse.ArgumentParser()
    parser.add_argument("-opt", type=str, help="Path to the options file.")
    args = parser.parse_args()
    with open(args.opt) as f:
        opt = yaml.safe_load(f)
    from .dp import init_distributed
    ctx = init_distributed()
    res = run_infer_scene(opt, rank=ctx.rank, world=ctx.world)
    print(f"rank {ctx.rank}: {res}")


if __name__ == "__main__":
    main()
