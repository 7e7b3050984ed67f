"""Raw Sentinel-2 L1C onto the model's grid: the statement of the grid, of the projection and of the warp, in NumPy float64 and 64-bit
integers.  No device, no HIP library: the inference path computes the same on the device (csrc/reproject.hip: `merc_to_utm_coords`,
`scene_warp`, `reproject_scene` of infer_scene.py) and is tested against this file.

THE GRID.  The model's pixels are Web-Mercator (EPSG:3857) at `MERC_PIXEL` = 2 pi R / 2^22 = 9.5546 m: global pixel (px, py) has its
origin at x = -pi R, y = +pi R and py grows southwards.  A zoom-17 tile `col_row` (the dataset's tile name) is the pixels
[32 col, 32 col + 32) x [32 row, 32 row + 32), one 32 x 32 chunk; a zoom-13 tile (one `infer_grid` tile, 16 x 16 chunks) is 512 pixels.

THE PROJECTION.  ESA ships L1C rasters in UTM (EPSG 326zz north, 327zz south).  `utm_from_lonlat` is the WGS84 transverse Mercator by
the Krueger series in the third flattening n through order 6 (Karney, "Transverse Mercator with an accuracy of a few nanometers",
J. Geodesy 2011, eqs. 7-12 and 35), k0 = 0.9996, false easting 500 000, false northing 10 000 000 in the south, central meridian
6 zone - 183.

THE WARP.  `source_coords` gives, for every pixel CENTRE of a window of the grid, the source pixel coordinates
u = (E - ULX) / XDIM - 0.5, v = (N - ULY) / YDIM - 0.5 in 16.16 fixed point, floor(u 65536 + 0.5), or the sentinel INT32_MIN in both
words where the centre falls outside -0.5 <= u < Ws - 0.5, -0.5 <= v < Hs - 0.5.  `warp_bilinear` is bilinear interpolation in
64-bit integers on those words, with the four neighbours clamped into the raster.

This is NOT what GDAL produces.  The reference's README sketches the same step as eleven lines of rasterio pseudo-code
(`reproject(..., resampling=Resampling.bilinear)` without a nodata value); GDAL behind it uses approximate transformers and its own
edge rules, and its bytes cannot be reproduced here.  The statement in this file is the definition of what this project computes.

GEOREFERENCE of a frame: `epsg`, `ulx`, `uly` (the outer corner of the upper-left pixel, metres), `xdim` > 0, `ydim` < 0 (metres per
pixel), `rows`, `cols`.  Read from `GRANULE/*/MTD_TL.xml` of a `.SAFE` product (`parse_mtd_tl`) or from a sidecar `NAME.json` with those
seven keys next to the raster (`read_sidecar`).  The element names of MTD_TL.xml - `HORIZONTAL_CS_CODE`, `Size resolution="10"` with
`NROWS` / `NCOLS`, `Geoposition resolution="10"` with `ULX` / `ULY` / `XDIM` / `YDIM` - are **[recalled]**: written from memory of
ESA's product specification, not checked against a product; tags are matched with any XML namespace.

Out of scope: the 16-bit band files, windows beyond 4096 pixels per side, georeferencing read out of JP2 / GeoTIFF boxes, source
projections other than UTM, agreement with GDAL's bytes."""
from __future__ import annotations

import glob
import json
import math
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np

R = 6378137.0                              # WGS84 semi-major axis = the sphere of EPSG:3857
WORLD = 1 << 22                            # pixels round the globe
MERC_PIXEL = 2.0 * math.pi * R / WORLD     # 9.554628535647032 m
TILE17, TILE13 = 32, 512                   # pixels per zoom-17 / zoom-13 tile
MAX_WINDOW = 4096                          # pixels per side of a window
FRAC_BITS = 16
ONE = 1 << FRAC_BITS                       # 1.0 in the coordinates' fixed point
INT32_MIN = -(1 << 31)                     # the sentinel: the centre lies outside the raster
MAX_RASTER = 32767                         # rows / cols of a source raster: its coordinates fit the 16.16 words
NODATA_MODES = ("blend", "propagate")

WGS84_F = 1.0 / 298.257223563
K0 = 0.9996
FALSE_EASTING, FALSE_NORTHING_SOUTH = 500000.0, 10000000.0


class Window(NamedTuple):
    """a window of the grid in global pixels: [px0, px0 + w) x [py0, py0 + h)"""
    px0: int
    py0: int
    w: int
    h: int


class Georef(NamedTuple):
    epsg: int
    ulx: float
    uly: float
    xdim: float
    ydim: float
    rows: int
    cols: int


GEOREF_KEYS = Georef._fields


# ------------------------------------------------------------------------------------------------ the projection
def utm_zone(epsg) -> Tuple[int, bool]:
    """(zone 1 .. 60, south) of a UTM EPSG code; every other code is refused by name"""
    if isinstance(epsg, bool) or not isinstance(epsg, (int, np.integer)) or not (32601 <= epsg <= 32660 or 32701 <= epsg <= 32760):
        raise ValueError(f"epsg = {epsg!r}: a WGS84 UTM code, 32601 .. 32660 (north) or 32701 .. 32760 (south)")
    epsg = int(epsg)
    return epsg % 100, epsg >= 32700


def kruger_series() -> Tuple[float, float, Tuple[float, ...]]:
    """(e, k0 A, (alpha_1 .. alpha_6)) of WGS84: the first eccentricity, the scaled rectifying radius and the coefficients of the
    forward series through n^6 (Karney 2011, eq. 35)"""
    f = WGS84_F
    n = f / (2.0 - f)
    e = math.sqrt(f * (2.0 - f))
    n2 = n * n
    A = R / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0)

    def poly(*c):                          # c[0] + c[1] n + ...
        s = 0.0
        for v in reversed(c):
            s = s * n + v
        return s

    alpha = (n * poly(1 / 2, -2 / 3, 5 / 16, 41 / 180, -127 / 288, 7891 / 37800),
             n ** 2 * poly(13 / 48, -3 / 5, 557 / 1440, 281 / 630, -1983433 / 1935360),
             n ** 3 * poly(61 / 240, -103 / 140, 15061 / 26880, 167603 / 181440),
             n ** 4 * poly(49561 / 161280, -179 / 168, 6601661 / 7257600),
             n ** 5 * poly(34729 / 80640, -3418889 / 1995840),
             n ** 6 * (212378941 / 319334400))
    return e, K0 * A, alpha


def utm_from_lonlat(lat, lon, epsg) -> Tuple[np.ndarray, np.ndarray]:
    """(easting, northing) in metres of geodetic latitude and longitude in DEGREES (WGS84) in the UTM zone of `epsg`"""
    zone, south = utm_zone(epsg)
    e, k0A, alpha = kruger_series()
    phi = np.radians(np.asarray(lat, np.float64))
    lam = np.radians(np.asarray(lon, np.float64) - (6.0 * zone - 183.0))
    tau = np.tan(phi)
    sigma = np.sinh(e * np.arctanh(e * tau / np.sqrt(1.0 + tau * tau)))
    taup = tau * np.sqrt(1.0 + sigma * sigma) - sigma * np.sqrt(1.0 + tau * tau)
    cl = np.cos(lam)
    xi0 = np.arctan2(taup, cl)
    eta0 = np.arcsinh(np.sin(lam) / np.sqrt(taup * taup + cl * cl))
    xi, eta = xi0, eta0
    for j, a in enumerate(alpha, 1):
        xi = xi + a * np.sin(2 * j * xi0) * np.cosh(2 * j * eta0)
        eta = eta + a * np.cos(2 * j * xi0) * np.sinh(2 * j * eta0)
    return FALSE_EASTING + k0A * eta, (FALSE_NORTHING_SOUTH if south else 0.0) + k0A * xi


def merc_pixel_to_lonlat(px, py) -> Tuple[np.ndarray, np.ndarray]:
    """(lon, lat) in degrees of the grid position (px, py) in global pixels; for a pixel pass its CENTRE, index + 0.5"""
    x = np.asarray(px, np.float64) * MERC_PIXEL - math.pi * R
    y = math.pi * R - np.asarray(py, np.float64) * MERC_PIXEL
    return np.degrees(x / R), np.degrees(np.arctan(np.sinh(y / R)))


def lonlat_to_merc_pixel(lon, lat) -> Tuple[np.ndarray, np.ndarray]:
    """the inverse of `merc_pixel_to_lonlat`: fractional global pixels (px, py) of a longitude and latitude in degrees"""
    x = R * np.radians(np.asarray(lon, np.float64))
    y = R * np.arcsinh(np.tan(np.radians(np.asarray(lat, np.float64))))
    return (x + math.pi * R) / MERC_PIXEL, (math.pi * R - y) / MERC_PIXEL


# ------------------------------------------------------------------------------------------------ windows
def tile_to_pixels(name: str, zoom: int) -> Window:
    """the tile `COL_ROW` of zoom 13 or 17 as a window"""
    if isinstance(zoom, bool) or zoom not in (13, 17):
        raise ValueError(f"window: zoom = {zoom!r}: 13 or 17")
    try:
        col, row = (int(v) for v in str(name).split("_"))
    except ValueError:
        raise ValueError(f"window: tile = {name!r}: a tile name COL_ROW") from None
    if not (0 <= col < 1 << zoom and 0 <= row < 1 << zoom):
        raise ValueError(f"window: tile = {name!r}: column and row from 0 to {(1 << zoom) - 1} at zoom {zoom}")
    side = TILE17 if zoom == 17 else TILE13
    return Window(side * col, side * row, side, side)


def pixels_to_tile(px: int, py: int, zoom: int) -> str:
    """the name `COL_ROW` of the zoom 13 or 17 tile that holds global pixel (px, py)"""
    if zoom not in (13, 17):
        raise ValueError(f"window: zoom = {zoom!r}: 13 or 17")
    side = TILE17 if zoom == 17 else TILE13
    return f"{int(px) // side}_{int(py) // side}"


def check_window(px0, py0, w, h) -> Window:
    vals = (px0, py0, w, h)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"window: pixels = {list(vals)}: four integers [px0, py0, w, h]")
    px0, py0, w, h = (int(v) for v in vals)
    if w % TILE17 or h % TILE17 or w < TILE17 or h < TILE17:
        raise ValueError(f"window: {w} x {h} pixels: width and height must be multiples of {TILE17}, at least {TILE17}")
    if w > MAX_WINDOW or h > MAX_WINDOW:
        raise ValueError(f"window: {w} x {h} pixels: at most {MAX_WINDOW} per side")
    if px0 < 0 or py0 < 0 or px0 + w > WORLD or py0 + h > WORLD:
        raise ValueError(f"window: pixels = {[px0, py0, w, h]} leave the grid of {WORLD} x {WORLD} pixels")
    return Window(px0, py0, w, h)


def parse_window(spec) -> Window:
    """`{tile: "COL_ROW", zoom: 13 | 17}`, `{pixels: [px0, py0, w, h]}` or `{bbox: [lon_min, lat_min, lon_max, lat_max]}` (degrees,
    snapped OUTWARDS to multiples of 32 pixels) -> Window.  Width and height are multiples of 32, at least 32 and at most 4096;
    everything else is refused by name."""
    if isinstance(spec, Window):
        return check_window(*spec)
    if not isinstance(spec, dict):
        raise ValueError(f"window = {spec!r}: a mapping with `tile` and `zoom`, `pixels` or `bbox`")
    kinds = [k for k in ("tile", "pixels", "bbox") if k in spec]
    extra = sorted(set(spec) - {"tile", "zoom", "pixels", "bbox"})
    if len(kinds) != 1 or extra or ("zoom" in spec) != (kinds == ["tile"]):
        raise ValueError(f"window = {spec!r}: exactly one of `tile` (with `zoom`), `pixels`, `bbox`")
    if kinds == ["tile"]:
        return check_window(*tile_to_pixels(spec["tile"], spec["zoom"]))
    if kinds == ["pixels"]:
        p = spec["pixels"]
        if not isinstance(p, (list, tuple)) or len(p) != 4:
            raise ValueError(f"window: pixels = {p!r}: four integers [px0, py0, w, h]")
        return check_window(*p)
    b = spec["bbox"]
    if not isinstance(b, (list, tuple)) or len(b) != 4 or any(isinstance(v, bool) or not isinstance(v, (int, float)) for v in b):
        raise ValueError(f"window: bbox = {b!r}: four numbers [lon_min, lat_min, lon_max, lat_max]")
    lon0, lat0, lon1, lat1 = (float(v) for v in b)
    if not (-180.0 <= lon0 < lon1 <= 180.0 and -85.0 <= lat0 < lat1 <= 85.0):
        raise ValueError(f"window: bbox = {b!r}: -180 <= lon_min < lon_max <= 180 and -85 <= lat_min < lat_max <= 85")
    (pxa, pxb), (pya, pyb) = lonlat_to_merc_pixel([lon0, lon1], [lat1, lat0])
    px0, py0 = int(math.floor(pxa / TILE17)) * TILE17, int(math.floor(pya / TILE17)) * TILE17
    px1, py1 = int(math.ceil(pxb / TILE17)) * TILE17, int(math.ceil(pyb / TILE17)) * TILE17
    return check_window(px0, py0, px1 - px0, py1 - py0)


def window_georef(window: Window, scale: int = 1) -> Dict:
    """what places a mosaic of the window in a GIS: EPSG 3857, the outer corner of the upper-left pixel in metres, the pixel size
    (MERC_PIXEL / scale) and the window in global pixels"""
    window = check_window(*window)
    return {"epsg": 3857, "ulx": window.px0 * MERC_PIXEL - math.pi * R, "uly": math.pi * R - window.py0 * MERC_PIXEL,
            "pixel_size": MERC_PIXEL / scale, "window_pixels": list(window)}


# ------------------------------------------------------------------------------------------------ georeferences
def check_georef(g) -> Georef:
    if isinstance(g, dict):
        missing = [k for k in GEOREF_KEYS if k not in g]
        if missing:
            raise ValueError(f"georeference {g!r}: missing {', '.join(missing)}")
        g = Georef(*(g[k] for k in GEOREF_KEYS))
    g = Georef(int(g.epsg), float(g.ulx), float(g.uly), float(g.xdim), float(g.ydim), int(g.rows), int(g.cols))
    utm_zone(g.epsg)
    if not (g.xdim > 0 and g.ydim < 0):
        raise ValueError(f"georeference: xdim = {g.xdim}, ydim = {g.ydim}: xdim > 0 and ydim < 0 (a north-up raster)")
    if not (1 <= g.rows <= MAX_RASTER and 1 <= g.cols <= MAX_RASTER):
        raise ValueError(f"georeference: {g.rows} x {g.cols} pixels: rows and cols from 1 to {MAX_RASTER}")
    return g


def _local(tag: str) -> str:
    return tag.rsplit("}", 1)[-1]


def parse_mtd_tl(path: str) -> Georef:
    """the 10 m georeference of a granule's MTD_TL.xml.  Element names [recalled] (see the module's docstring); tags are matched
    whatever their namespace."""
    import xml.etree.ElementTree as ET
    root = ET.parse(path).getroot()
    found: Dict[str, str] = {}
    for el in root.iter():
        name = _local(el.tag)
        if name == "HORIZONTAL_CS_CODE" and el.text:
            found["epsg"] = el.text.strip().upper().replace("EPSG:", "")
        elif name in ("Size", "Geoposition") and el.get("resolution") == "10":
            for c in el:
                if c.text:
                    found[_local(c.tag).lower()] = c.text.strip()
    want = {"epsg": "HORIZONTAL_CS_CODE", "nrows": 'Size resolution="10"/NROWS', "ncols": 'Size resolution="10"/NCOLS',
            "ulx": 'Geoposition resolution="10"/ULX', "uly": 'Geoposition resolution="10"/ULY',
            "xdim": 'Geoposition resolution="10"/XDIM', "ydim": 'Geoposition resolution="10"/YDIM'}
    missing = [v for k, v in want.items() if k not in found]
    if missing:
        raise ValueError(f"{path}: no {', '.join(missing)}")
    try:
        return check_georef(Georef(int(found["epsg"]), float(found["ulx"]), float(found["uly"]), float(found["xdim"]),
                                   float(found["ydim"]), int(found["nrows"]), int(found["ncols"])))
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def read_sidecar(path: str) -> Georef:
    """the georeference of a sidecar file NAME.json: the seven keys epsg, ulx, uly, xdim, ydim, rows, cols"""
    with open(path) as f:
        d = json.load(f)
    try:
        if not isinstance(d, dict):
            raise ValueError(f"a mapping with the keys {', '.join(GEOREF_KEYS)}")
        return check_georef(d)
    except (ValueError, TypeError) as e:
        raise ValueError(f"{path}: {e}") from None


RASTER_EXTS = (".jp2", ".tif", ".tiff", ".png", ".npy")


def find_product(path: str) -> Tuple[str, Georef]:
    """(raster file, georeference) of one product: a `.SAFE` directory (its `*_TCI.jp2` under GRANULE/*/IMG_DATA/, its georeference
    from GRANULE/*/MTD_TL.xml) or a raster file with its sidecar NAME.json beside it"""
    if os.path.isdir(path):
        tci = sorted(glob.glob(os.path.join(path, "GRANULE", "*", "IMG_DATA", "*_TCI.jp2")))
        if len(tci) != 1:
            raise ValueError(f"{path}: {len(tci)} files GRANULE/*/IMG_DATA/*_TCI.jp2, expected one")
        mtd = os.path.join(os.path.dirname(os.path.dirname(tci[0])), "MTD_TL.xml")
        if not os.path.isfile(mtd):
            raise ValueError(f"{path}: no {os.path.relpath(mtd, path)}")
        return tci[0], parse_mtd_tl(mtd)
    side = os.path.splitext(path)[0] + ".json"
    if not os.path.isfile(side):
        raise ValueError(f"{path}: no sidecar {os.path.basename(side)} with the keys {', '.join(GEOREF_KEYS)}")
    return path, read_sidecar(side)


def list_products(scene_dir: str) -> Sequence[str]:
    """the products of a scene directory, sorted by name: `.SAFE` directories and raster files (.jp2 / .tif / .png / .npy)"""
    out = []
    for f in sorted(os.listdir(scene_dir)):
        p = os.path.join(scene_dir, f)
        if (os.path.isdir(p) and f.upper().endswith(".SAFE")) or (os.path.isfile(p) and os.path.splitext(f)[1].lower() in RASTER_EXTS):
            out.append(p)
    return out


# ------------------------------------------------------------------------------------------------ coordinates and the warp
def _source_uv(px, py, g: Georef) -> Tuple[np.ndarray, np.ndarray]:
    """float64 source pixel coordinates (u, v) of the grid positions (px, py) (centres: index + 0.5)"""
    lon, lat = merc_pixel_to_lonlat(px, py)
    E, N = utm_from_lonlat(lat, lon, g.epsg)
    return (E - g.ulx) / g.xdim - 0.5, (N - g.uly) / g.ydim - 0.5


def source_coords(window, georef) -> np.ndarray:
    """int32 [h, w, 2]: (U, V) of every pixel centre of the window, floor(u 65536 + 0.5) and floor(v 65536 + 0.5) with
    u = (E - ULX) / XDIM - 0.5, v = (N - ULY) / YDIM - 0.5; both words INT32_MIN where the centre falls outside
    -0.5 <= u < cols - 0.5, -0.5 <= v < rows - 0.5"""
    window, g = parse_window(window), check_georef(georef)
    px = window.px0 + np.arange(window.w, dtype=np.float64) + 0.5
    py = window.py0 + np.arange(window.h, dtype=np.float64) + 0.5
    u, v = _source_uv(px[None, :], py[:, None], g)
    with np.errstate(invalid="ignore"):
        inside = (u >= -0.5) & (u < g.cols - 0.5) & (v >= -0.5) & (v < g.rows - 0.5)
    out = np.full((window.h, window.w, 2), INT32_MIN, np.int64)
    out[..., 0][inside] = np.floor(u[inside] * ONE + 0.5)
    out[..., 1][inside] = np.floor(v[inside] * ONE + 0.5)
    return out.astype(np.int32)


def warp_bilinear(src: np.ndarray, coords: np.ndarray, nodata: str = "blend") -> np.ndarray:
    """src uint8 [T, Hs, Ws, C] (C = 1 or 3), coords int32 [h, w, 2] (`source_coords`) -> uint8 [T, h, w, C].
    x0 = U >> 16 (arithmetic), fx = U & 0xffff, likewise y; the four neighbours clamped into the raster;
    out = ((65536 - fx)(65536 - fy) p00 + fx (65536 - fy) p10 + (65536 - fx) fy p01 + fx fy p11 + 2^31) >> 32 in 64-bit integers.
    A sentinel coordinate (both words INT32_MIN) gives 0 in every channel.
    nodata "blend" is plain bilinear (what the reference's pseudo-code asks of GDAL, which gets no nodata value).  "propagate" is
    this project's own policy: where a neighbour with NON-ZERO weight has a zero among its C samples (ESA's NODATA) the output
    pixel is 0 in every channel, so NODATA stays NODATA for `frame_select: clearest` and `nodata: keep` behind the warp instead
    of becoming a dark fringe of blended values."""
    src, coords = np.asarray(src), np.asarray(coords)
    if src.dtype != np.uint8 or src.ndim != 4 or src.shape[3] not in (1, 3) or 0 in src.shape:
        raise ValueError(f"a source is a uint8 array [T, Hs, Ws, C] with C = 1 or 3, not {src.dtype} {tuple(src.shape)}")
    if coords.dtype != np.int32 or coords.ndim != 3 or coords.shape[2] != 2:
        raise ValueError(f"coordinates are an int32 array [h, w, 2], not {coords.dtype} {tuple(coords.shape)}")
    if nodata not in NODATA_MODES:
        raise ValueError(f"reproject_nodata = {nodata!r}: one of {', '.join(NODATA_MODES)}")
    _, Hs, Ws, _ = src.shape
    U, V = coords[..., 0].astype(np.int64), coords[..., 1].astype(np.int64)
    sentinel = (U == INT32_MIN) & (V == INT32_MIN)
    x0, y0, fx, fy = U >> FRAC_BITS, V >> FRAC_BITS, U & (ONE - 1), V & (ONE - 1)
    xa, xb = np.clip(x0, 0, Ws - 1), np.clip(x0 + 1, 0, Ws - 1)
    ya, yb = np.clip(y0, 0, Hs - 1), np.clip(y0 + 1, 0, Hs - 1)
    w00, w10, w01, w11 = (ONE - fx) * (ONE - fy), fx * (ONE - fy), (ONE - fx) * fy, fx * fy
    acc = np.full(src.shape[:1] + U.shape + src.shape[3:], 1 << 31, np.int64)
    dead = np.zeros(src.shape[:1] + U.shape, bool)
    for wgt, yy, xx in ((w00, ya, xa), (w10, ya, xb), (w01, yb, xa), (w11, yb, xb)):
        p = src[:, yy, xx]                                     # [T, h, w, C]
        acc += wgt[None, :, :, None] * p.astype(np.int64)
        dead |= (wgt != 0)[None] & (p == 0).any(axis=-1)
    out = (acc >> 32).astype(np.uint8)
    out[:, sentinel] = 0
    if nodata == "propagate":
        out[dead] = 0
    return out


def source_crop(window, georef, pad: int = 2) -> Optional[Tuple[int, int, int, int]]:
    """(x0, y0, x1, y1): the source rectangle [x0, x1) x [y0, y1) the window needs, or None where the window misses the raster.
    The source coordinates are evaluated along the window's border (the map is continuous and one-to-one, so the border's bounding
    box bounds the interior's), padded by `pad` pixels and cut to the raster."""
    window, g = parse_window(window), check_georef(georef)
    xs = window.px0 + np.arange(window.w, dtype=np.float64) + 0.5
    ys = window.py0 + np.arange(window.h, dtype=np.float64) + 0.5
    bx = np.concatenate([xs, xs, np.full(window.h, xs[0]), np.full(window.h, xs[-1])])
    by = np.concatenate([np.full(window.w, ys[0]), np.full(window.w, ys[-1]), ys, ys])
    u, v = _source_uv(bx, by, g)
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        return None
    x0, x1 = max(0, int(math.floor(u.min())) - pad), min(g.cols, int(math.floor(u.max())) + 2 + pad)
    y0, y1 = max(0, int(math.floor(v.min())) - pad), min(g.rows, int(math.floor(v.max())) + 2 + pad)
    if x0 >= x1 or y0 >= y1:
        return None
    return x0, y0, x1, y1


def crop_georef(georef, box: Tuple[int, int, int, int]) -> Georef:
    """the georeference of the crop [x0, x1) x [y0, y1) of a raster: its own ulx / uly, rows and cols"""
    g = check_georef(georef)
    x0, y0, x1, y1 = box
    assert 0 <= x0 < x1 <= g.cols and 0 <= y0 < y1 <= g.rows, (box, g)
    return g._replace(ulx=g.ulx + x0 * g.xdim, uly=g.uly + y0 * g.ydim, rows=y1 - y0, cols=x1 - x0)


def reproject_reference(rasters, georefs, window, nodata: str = "blend") -> np.ndarray:
    """The whole step on the CPU, frame by frame on the FULL rasters: uint8 [T, h, w, C].  rasters: T arrays uint8 [Hs, Ws, C]
    (or [Hs, Ws]), georefs: their georeferences."""
    window = parse_window(window)
    out = []
    for a, g in zip(rasters, georefs):
        a = np.asarray(a)
        a = a[:, :, None] if a.ndim == 2 else a
        out.append(warp_bilinear(a[None], source_coords(window, g), nodata)[0])
    return np.stack(out)
