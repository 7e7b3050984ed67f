"""What the reprojection in front of scene inference costs (`source: sentinel2_l1c`), on ONE GPU, in one process:

  a 512 x 512 window at the equator (zone 31), T = 8 frames whose source crops (about 495 x 495 pixels of 10 m, one georeference)
  are RESIDENT on the device; SSR_RRDBNet(24, 3, 4, 64, 23, 32) with random weights, n_lr_images 8, batch 64.

  (a) `merc_to_utm_coords` -> `scene_warp` -> `super_resolve_scene` on the warped tensor, each of the three between HIP events;
  (b) `super_resolve_scene` fed an already-warped tensor - the path without the option;
  the two alternate five times after a warm-up of each.  Nothing is tuned and nothing is gated: the numbers are written down.

  The host's decode is timed apart (`--decode SIDE`, default 10980, 0 to skip): one lossless JP2 and one TIFF of SIDE x SIDE pixels
  are written to a temporary directory and `png_io.read_raster_crop` reads the window's rectangle out of each, three times.  Pillow
  decodes the file whole, so this is the cost per product whatever the window.

    python tools/scene_reproject_bench.py [mode] [--decode SIDE] > profiles/scene_reproject/bench.json
"""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def _field(rng, H, W, T=None):
    """smooth field + noise, no black samples"""
    yy, xx = np.mgrid[0:H, 0:W]
    base = 110 + 60 * np.sin(yy / 19.0)[:, :, None] * np.cos(xx / 11.0)[:, :, None]
    shape = (H, W, 3) if T is None else (T, H, W, 3)
    return np.clip(base + rng.randint(-12, 13, shape), 1, 255).astype(np.uint8)


def _site(side):
    """the window and a raster of side x side pixels of 10 m whose pixel (8, 8) holds the window's upper-left corner"""
    from satlas_super_resolution_amd import s2_reproject as S
    px, py = S.lonlat_to_merc_pixel(5.5, 0.5)
    win = S.Window(int(px) // 32 * 32, int(py) // 32 * 32, 512, 512)
    lon, lat = S.merc_pixel_to_lonlat(float(win.px0), float(win.py0))
    e, n = (float(v) for v in S.utm_from_lonlat(lat, lon, 32631))
    return win, S.Georef(32631, e // 10 * 10 - 80.0, -(-n // 10) * 10 + 80.0, 10.0, -10.0, side, side)


def decode_leg(side):
    from PIL import Image
    from satlas_super_resolution_amd import png_io, s2_reproject as S
    win, g = _site(side)
    box = S.source_crop(win, g)
    tmp = tempfile.mkdtemp(prefix="reproject_bench_")
    try:
        img = Image.fromarray(_field(np.random.RandomState(1), side, side))
        out = {"pixels": [side, side], "crop_box": list(box), "decoders": png_io.raster_decoders()}
        with png_io._pixel_limit():
            for name, kw in (("tci.jp2", {"irreversible": False}), ("tci.tif", {})):
                path = os.path.join(tmp, name)
                t0 = time.perf_counter()
                img.save(path, **kw)
                enc = time.perf_counter() - t0
                secs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    a = png_io.read_raster_crop(path, box)
                    secs.append(time.perf_counter() - t0)
                assert a.shape == (box[3] - box[1], box[2] - box[0], 3)
                out[name] = {"file_bytes": os.path.getsize(path), "encode_seconds": enc, "decode_seconds": secs,
                             "median": statistics.median(secs), "spread": max(secs) - min(secs)}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    argv = sys.argv[1:]
    side = 10980
    if "--decode" in argv:
        k = argv.index("--decode")
        side = int(argv[k + 1])
        argv = argv[:k] + argv[k + 2:]
    mode = argv[0] if argv else "fp32h"
    from satlas_super_resolution_amd import s2_reproject as S
    from satlas_super_resolution_amd.archs.rrdbnet_arch import SSR_RRDBNet
    from satlas_super_resolution_amd.infer_scene import merc_to_utm_coords, scene_warp, super_resolve_scene
    T = 8
    win, g = _site(640)
    box = S.source_crop(win, g)
    gc = S.crop_georef(g, box)
    crops = torch.from_numpy(_field(np.random.RandomState(0), gc.rows, gc.cols, T)).cuda()      # resident: no upload is timed
    net = SSR_RRDBNet(24, 3, 4, 64, 23, 32, compute_dtype=mode).cuda().eval().freeze_packed()
    coords = torch.empty(win.h, win.w, 2, dtype=torch.int32, device="cuda")
    warped = torch.empty(T, win.h, win.w, 3, dtype=torch.uint8, device="cuda")
    ready = scene_warp(crops, merc_to_utm_coords(win, gc), "blend").clone()                   # (b)'s input: made once

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def with_reprojection():
        e = [ev() for _ in range(4)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        merc_to_utm_coords(win, gc, out=coords)
        e[1].record()
        scene_warp(crops, coords, "blend", warped)
        e[2].record()
        super_resolve_scene(net, warped, 8, frame_select="clearest")
        e[3].record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return {"coords_ms": e[0].elapsed_time(e[1]), "warp_ms": e[1].elapsed_time(e[2]), "scene_ms": e[2].elapsed_time(e[3]),
                "wall_ms": 1e3 * wall}

    def already_warped():
        e = [ev(), ev()]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e[0].record()
        super_resolve_scene(net, ready, 8, frame_select="clearest")
        e[1].record()
        torch.cuda.synchronize()
        return {"scene_ms": e[0].elapsed_time(e[1]), "wall_ms": 1e3 * (time.perf_counter() - t0)}

    warm = [with_reprojection(), already_warped()]      # plans, graph capture, first touch
    a, b = [], []
    for _ in range(5):
        a.append(with_reprojection())
        b.append(already_warped())
    assert torch.equal(warped, ready)

    def stats(rows, key):
        v = [r[key] for r in rows]
        return {"values": v, "median": statistics.median(v), "min": min(v), "spread": max(v) - min(v)}

    rec = {"workload": "512 x 512 window at the equator, 8 frames, source crops of %d x %d pixels resident on the device, one "
                       "georeference; SSR_RRDBNet(nf=64, nb=23, gc=32), random weights, n_lr_images 8, batch 64, frame_select clearest, "
                       "one GPU; HIP events round each stage, the two paths alternate in one process" % (gc.rows, gc.cols),
           "device": torch.cuda.get_device_name(0), "compute_dtype": mode, "warm_up": warm,
           "with_reprojection": {k: stats(a, k) for k in ("coords_ms", "warp_ms", "scene_ms", "wall_ms")},
           "already_warped": {k: stats(b, k) for k in ("scene_ms", "wall_ms")}}
    rec["reprojection_share_of_scene"] = (rec["with_reprojection"]["coords_ms"]["median"] + rec["with_reprojection"]["warp_ms"]["median"]) \
        / rec["already_warped"]["scene_ms"]["median"]
    if side:
        rec["host_decode_per_product"] = decode_leg(side)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
