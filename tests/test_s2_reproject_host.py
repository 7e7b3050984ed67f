"""CPU: the statement of the Sentinel-2 reprojection (satlas_super_resolution_amd/s2_reproject.py) - the projection against facts
that do not come from the code (a published easting, the meridian arc integrated numerically, the Cauchy-Riemann equations of a
conformal map), the grid and its refusals, the integer warp on cases worked out by hand, the two georeference parsers and the crop
helper.  No device and no HIP library."""
import json
import math

import numpy as np
import pytest

from satlas_super_resolution_amd import s2_reproject as S

A, F = 6378137.0, 1 / 298.257223563
E2 = F * (2 - F)


# ---------------------------------------------------------------- 1. the projection
@pytest.mark.parametrize("zone", [1, 31, 60])
def test_equator_three_degrees_from_the_meridian(zone):
    """833 978.557 m: the easting of the zone edge on the equator"""
    cm = 6 * zone - 183
    e, n = S.utm_from_lonlat(0.0, cm + 3, 32600 + zone)
    print(f"zone {zone}: easting {float(e):.6f} northing {float(n):.3e}")
    assert abs(float(e) - 833978.557) < 1e-3 and abs(float(n)) < 1e-9
    e, n = S.utm_from_lonlat(0.0, cm - 3, 32600 + zone)
    assert abs(float(e) - (1000000 - 833978.557)) < 1e-3


@pytest.mark.filterwarnings("ignore::scipy.integrate.IntegrationWarning")      # (at 84 degrees 1e-7 m of 9e6 m is close to fp64's limit)
@pytest.mark.parametrize("lat", [10.0, 45.0, 60.0, 84.0])
def test_northing_on_the_central_meridian_is_the_scaled_meridian_arc(lat):
    from scipy.integrate import quad
    arc, _ = quad(lambda p: A * (1 - E2) / (1 - E2 * math.sin(p) ** 2) ** 1.5, 0.0, math.radians(lat), epsabs=1e-7, epsrel=0)
    e, n = S.utm_from_lonlat(lat, 15.0, 32633)
    print(f"lat {lat}: northing {float(n):.9f}, 0.9996 arc {0.9996 * arc:.9f}, difference {abs(float(n) - 0.9996 * arc):.2e} m")
    assert abs(float(n) - 0.9996 * arc) < 1e-6
    assert abs(float(e) - 500000.0) < 1e-9


@pytest.mark.parametrize("lat,dlon", [(0.1, 2.99), (47.6, -1.0), (-33.9, 4.0), (83.5, -4.0), (60.0, 0.0)])
def test_the_map_is_conformal(lat, dlon):
    """Cauchy-Riemann in the isometric latitude psi: dE/dlambda = dN/dpsi and dE/dpsi = -dN/dlambda.  Central differences with a step
    of 1e-6 rad (6 m): truncation ~ h^2 |f'''| / 6 ~ 1e-12 R, rounding ~ 1e-9 m / h = 1e-3 m per radian; against derivatives of
    ~ 6e6 m per radian the bound 1 m per radian is 2e-7 relative."""
    lon0 = 15.0
    h = 1e-6

    def psi(phi):
        return math.asinh(math.tan(phi)) - math.sqrt(E2) * math.atanh(math.sqrt(E2) * math.sin(phi))

    phi = math.radians(lat)
    dpsi_dphi = (psi(phi + h) - psi(phi - h)) / (2 * h)
    f = lambda p, l: tuple(float(v) for v in S.utm_from_lonlat(math.degrees(p), lon0 + dlon + math.degrees(l), 32633))
    (e1, n1), (e0, n0) = f(phi, h), f(phi, -h)
    dE_dl, dN_dl = (e1 - e0) / (2 * h), (n1 - n0) / (2 * h)
    (e1, n1), (e0, n0) = f(phi + h, 0.0), f(phi - h, 0.0)
    dE_dpsi, dN_dpsi = (e1 - e0) / (2 * h) / dpsi_dphi, (n1 - n0) / (2 * h) / dpsi_dphi
    print(f"lat {lat} dlon {dlon}: dE/dl {dE_dl:.3f} dN/dpsi {dN_dpsi:.3f}  dE/dpsi {dE_dpsi:.3f} -dN/dl {-dN_dl:.3f}")
    assert abs(dE_dl - dN_dpsi) < 1.0 and abs(dE_dpsi + dN_dl) < 1.0
    assert abs(dE_dl) > 1e5


def test_southern_false_northing_and_refusals():
    en, nn = S.utm_from_lonlat(-33.9, 151.2, 32656)
    es, ns = S.utm_from_lonlat(-33.9, 151.2, 32756)
    assert float(es) == float(en) and float(ns) - float(nn) == 10000000.0 and float(nn) < 0 < float(ns)
    assert S.utm_zone(32756) == (56, True) and S.utm_zone(32601) == (1, False)
    for bad in (3857, 4326, 32600, 32661, 32700, 32761, "32631", True, 32631.0):
        with pytest.raises(ValueError, match="epsg"):
            S.utm_from_lonlat(0.0, 0.0, bad)


def test_kruger_coefficients_lead_with_the_known_terms():
    e, k0A, alpha = S.kruger_series()
    assert abs(e * e - E2) < 1e-18 and len(alpha) == 6
    assert abs(k0A / 0.9996 - 6367449.145823) < 1e-5          # the rectifying radius of WGS84
    assert abs(alpha[0] - 8.377318206245e-4) < 1e-15 and abs(alpha[1] - 7.608527773572e-7) < 1e-18


# ---------------------------------------------------------------- 2. the grid
def test_pixel_size_and_mercator_round_trip():
    assert S.MERC_PIXEL == 9.554628535647032 == 2 * math.pi * S.R / 2 ** 22
    lon, lat = S.merc_pixel_to_lonlat(2 ** 21, 2 ** 21)
    assert float(lon) == 0.0 and float(lat) == 0.0
    lon, lat = S.merc_pixel_to_lonlat(0.0, 0.0)
    assert abs(float(lon) + 180.0) < 1e-12 and abs(float(lat) - 85.0511287798066) < 1e-12
    px, py = S.lonlat_to_merc_pixel(*S.merc_pixel_to_lonlat(np.array([1234567.5]), np.array([2345678.5])))
    assert abs(px[0] - 1234567.5) < 1e-6 and abs(py[0] - 2345678.5) < 1e-6
    _, lat_n = S.merc_pixel_to_lonlat(0.5, 100.5)
    _, lat_s = S.merc_pixel_to_lonlat(0.5, 101.5)
    assert float(lat_s) < float(lat_n)                               # py grows southwards


def test_tile_names_and_pixels():
    assert S.parse_window({"tile": "5_7", "zoom": 17}) == S.Window(160, 224, 32, 32)
    assert S.parse_window({"tile": "5_7", "zoom": 13}) == S.Window(2560, 3584, 512, 512)
    assert S.parse_window({"tile": f"{2 ** 17 - 1}_{2 ** 17 - 1}", "zoom": 17}) == S.Window(2 ** 22 - 32, 2 ** 22 - 32, 32, 32)
    assert S.pixels_to_tile(160 + 31, 224, 17) == "5_7" and S.pixels_to_tile(192, 224, 17) == "6_7"
    assert S.pixels_to_tile(2560 + 511, 3584 + 511, 13) == "5_7"
    w = S.parse_window({"tile": "4321_2765", "zoom": 13})
    assert S.pixels_to_tile(w.px0, w.py0, 13) == "4321_2765" and S.pixels_to_tile(w.px0, w.py0, 17) == f"{4321 * 16}_{2765 * 16}"
    assert S.parse_window({"pixels": [64, 96, 4096, 32]}) == S.Window(64, 96, 4096, 32)
    g = S.window_georef(S.Window(2 ** 21, 2 ** 21 - 32, 64, 32), 4)
    assert sorted(g) == ["epsg", "pixel_size", "ulx", "uly", "window_pixels"]
    assert g["epsg"] == 3857 and g["pixel_size"] == S.MERC_PIXEL / 4 and g["window_pixels"] == [2 ** 21, 2 ** 21 - 32, 64, 32]
    assert abs(g["ulx"]) < 1e-6 and abs(g["uly"] - 32 * S.MERC_PIXEL) < 1e-6


def test_bbox_snaps_outwards_to_multiples_of_32():
    bbox = [2.90, 0.05, 2.95, 0.10]
    w = S.parse_window({"bbox": bbox})
    assert w.px0 % 32 == 0 and w.py0 % 32 == 0 and w.w % 32 == 0 and w.h % 32 == 0
    (pxa, pxb), (pya, pyb) = S.lonlat_to_merc_pixel([bbox[0], bbox[2]], [bbox[3], bbox[1]])
    assert w.px0 <= pxa < w.px0 + 32 and w.px0 + w.w - 32 < pxb <= w.px0 + w.w
    assert w.py0 <= pya < w.py0 + 32 and w.py0 + w.h - 32 < pyb <= w.py0 + w.h
    lon, lat = S.merc_pixel_to_lonlat(np.array([w.px0, w.px0 + w.w], float), np.array([w.py0, w.py0 + w.h], float))
    assert lon[0] <= bbox[0] and lon[1] >= bbox[2] and lat[0] >= bbox[3] and lat[1] <= bbox[1]
    # a box that is a tile exactly stays that tile
    t = S.parse_window({"tile": "70000_60000", "zoom": 17})
    lon, lat = S.merc_pixel_to_lonlat(np.array([t.px0 + 0.25, t.px0 + 31.75]), np.array([t.py0 + 0.25, t.py0 + 31.75]))
    assert S.parse_window({"bbox": [lon[0], lat[1], lon[1], lat[0]]}) == t


@pytest.mark.parametrize("spec", [
    None, [0, 0, 32, 32], {}, {"pixels": [0, 0, 32, 32], "bbox": [0, 0, 1, 1]}, {"pixels": [0, 0, 32, 32], "zoom": 17},
    {"tile": "5_7"}, {"tile": "5_7", "zoom": 12}, {"tile": "5_7", "zoom": True}, {"tile": "5-7", "zoom": 17}, {"tile": "5_x", "zoom": 17},
    {"tile": f"{2 ** 17}_0", "zoom": 17}, {"tile": "-1_0", "zoom": 13}, {"tile": "5_7", "zoom": 17, "level": 1},
    {"pixels": [0, 0, 32]}, {"pixels": [0, 0, 32.0, 32]}, {"pixels": [0, 0, True, 32]}, {"pixels": "0 0 32 32"},
    {"pixels": [0, 0, 0, 32]}, {"pixels": [0, 0, 48, 32]}, {"pixels": [0, 0, 32, 33]}, {"pixels": [0, 0, 4128, 32]},
    {"pixels": [0, 0, 32, 8192]}, {"pixels": [-32, 0, 32, 32]}, {"pixels": [2 ** 22 - 32, 0, 64, 32]}, {"pixels": [0, 2 ** 22, 32, 32]},
    {"bbox": [0, 0, 1]}, {"bbox": [1, 0, 0, 1]}, {"bbox": [0, 1, 1, 0]}, {"bbox": [0, 0, 1, 86]}, {"bbox": [-181, 0, 1, 1]},
    {"bbox": [0, 0, "1", 1]}, {"bbox": [0.0, 0.0, 1.0, 1.0]},          # (the last: 1 degree is ~ 11 650 pixels, above 4096 per side)
])
def test_window_refusals(spec):
    with pytest.raises(ValueError, match="window"):
        S.parse_window(spec)


# ---------------------------------------------------------------- 3. the warp
def _coords(u, v):
    """int32 [h, w, 2] from exact fixed-point positions given in pixels"""
    u, v = np.broadcast_arrays(np.asarray(u, float), np.asarray(v, float))
    return np.stack([np.floor(u * 65536 + 0.5), np.floor(v * 65536 + 0.5)], -1).astype(np.int32)


def _src(T=2, Hs=9, Ws=11, C=3, seed=0):
    return np.random.RandomState(seed).randint(1, 256, size=(T, Hs, Ws, C)).astype(np.uint8)


@pytest.mark.parametrize("C", [1, 3])
def test_a_whole_pixel_translation_is_a_crop(C):
    src = _src(C=C)
    yy, xx = np.mgrid[0:4, 0:5]
    out = S.warp_bilinear(src, _coords(xx + 3, yy + 2))
    assert out.dtype == np.uint8 and np.array_equal(out, src[:, 2:6, 3:8])
    assert np.array_equal(S.warp_bilinear(src, _coords(xx + 3, yy + 2), "propagate"), src[:, 2:6, 3:8])


def test_half_pixel_offsets_are_rounded_means():
    src = _src(T=1, C=3, seed=1)
    s = src.astype(np.int64)
    yy, xx = np.mgrid[0:4, 0:5]
    out = S.warp_bilinear(src, _coords(xx + 3.5, yy + 2))
    assert np.array_equal(out, ((s[:, 2:6, 3:8] + s[:, 2:6, 4:9] + 1) >> 1))            # a tie rounds up (+ 2^31)
    out = S.warp_bilinear(src, _coords(xx + 3, yy + 2.5))
    assert np.array_equal(out, ((s[:, 2:6, 3:8] + s[:, 3:7, 3:8] + 1) >> 1))
    out = S.warp_bilinear(src, _coords(xx + 3.5, yy + 2.5))
    assert np.array_equal(out, ((s[:, 2:6, 3:8] + s[:, 2:6, 4:9] + s[:, 3:7, 3:8] + s[:, 3:7, 4:9] + 2) >> 2))
    # a quarter: weights 3/4 and 1/4
    out = S.warp_bilinear(src, _coords(xx + 3.25, yy + 2))
    assert np.array_equal(out, ((3 * s[:, 2:6, 3:8] + s[:, 2:6, 4:9] + 2) >> 2))


def test_the_outermost_half_pixel_uses_clamped_neighbours_and_the_sentinel_gives_zero():
    src = _src(T=1, Hs=4, Ws=5, C=3, seed=2)
    c = _coords([[-0.5, 4.25, 2.0, -0.25]], [[0.0, 3.4, -0.5, 3.49]])
    out = S.warp_bilinear(src, c)[0, 0]
    assert np.array_equal(out[0], src[0, 0, 0])                      # x0 = -1 and x0 + 1 = 0 both clamp to column 0
    assert np.array_equal(out[1], src[0, 3, 4])                      # right and bottom: both neighbours are the last pixel
    assert np.array_equal(out[2], src[0, 0, 2])                      # y0 = -1 and 0 clamp to row 0
    assert np.array_equal(out[3], src[0, 3, 0])
    assert (c[0, 0] == [-32768, 0]).all() and (c[0, 0, 0] >> 16) == -1 and (c[0, 0, 0] & 0xffff) == 32768
    c[0, 2] = S.INT32_MIN
    out = S.warp_bilinear(src, c)[0, 0]
    assert (out[2] == 0).all() and (out[[0, 1, 3]] != 0).all()
    c[0, 1, 1] = S.INT32_MIN                                         # one word alone is no sentinel: a coordinate, clamped
    assert np.array_equal(S.warp_bilinear(src, c)[0, 0, 1], src[0, 0, 4])


def test_propagate_zeroes_exactly_the_pixels_that_touch_a_zero_with_weight():
    src = _src(T=2, Hs=6, Ws=6, C=3, seed=3)
    src[0, 2, 3, 1] = 0                                              # one zero SAMPLE of frame 0's pixel (row 2, column 3)
    u = np.array([[3.0, 2.0, 2.5, 3.5, 4.0, 3.0, 3.0, 2.5, 2.999985, 3.000015]])
    v = np.array([[2.0, 2.0, 2.0, 2.0, 2.0, 1.5, 3.0, 1.5, 1.0, 2.0]])
    touches = np.array([1, 0, 1, 1, 0, 1, 0, 1, 0, 1], bool)         # (2, 2) and (4, 2): weight 0 on column 3; (2.999985, 1): row 2 has weight 0
    c = _coords(u, v)
    assert (c[0, 8, 0] & 0xffff) == 65535 and (c[0, 9, 0] & 0xffff) == 1
    blend, prop = S.warp_bilinear(src, c), S.warp_bilinear(src, c, "propagate")
    assert np.array_equal(prop[1], blend[1])                         # frame 1 holds no zero
    assert ((prop[0, 0] == 0).all(axis=-1) == touches).all()
    assert np.array_equal(prop[0, 0][~touches], blend[0, 0][~touches])
    assert (blend[0, 0][[2, 3, 5, 7, 9]] != 0).any(axis=-1).all()      # blend makes a dark fringe there, not NODATA
    gray = src[..., 1:2].copy()
    assert ((S.warp_bilinear(gray, c, "propagate")[0, 0, :, 0] == 0) == touches).all()


def test_warp_refusals():
    src, c = _src(), _coords(np.zeros((2, 2)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="reproject_nodata"):
        S.warp_bilinear(src, c, "mask")
    with pytest.raises(ValueError, match="source"):
        S.warp_bilinear(src[..., :2], c)
    with pytest.raises(ValueError, match="source"):
        S.warp_bilinear(src.astype(np.uint16), c)
    with pytest.raises(ValueError, match="coordinates"):
        S.warp_bilinear(src, c.astype(np.int64))


# ---------------------------------------------------------------- 4. coordinates, parsers and the crop
GEOREF = S.Georef(32631, 799980.0, 100020.0, 10.0, -10.0, 300, 400)      # a raster at the eastern edge of zone 31, just north of the equator


def _window_at(e, n, epsg, w, h):
    """a window whose upper-left pixel holds the UTM point (e, n): found by bisection-free inversion through a coarse search"""
    zone, south = S.utm_zone(epsg)
    lon, lat = 6 * zone - 183 + 0.0, -1.0 if south else 1.0
    for _ in range(60):                                              # Newton on the forward map (well conditioned inside a zone)
        e0, n0 = (float(v) for v in S.utm_from_lonlat(lat, lon, epsg))
        lat += (n - n0) / 111000.0
        lon += (e - e0) / (111000.0 * math.cos(math.radians(lat)))
    px, py = S.lonlat_to_merc_pixel(lon, lat)
    return S.Window(int(px), int(py), w, h)


def test_source_coords_are_the_fixed_point_positions_and_the_sentinel():
    win = _window_at(GEOREF.ulx + 500.0, GEOREF.uly - 400.0, GEOREF.epsg, 64, 96)
    c = S.source_coords(win, GEOREF)
    assert c.dtype == np.int32 and c.shape == (96, 64, 2) and (c != S.INT32_MIN).all()
    lon, lat = S.merc_pixel_to_lonlat(win.px0 + 10.5, win.py0 + 20.5)
    e, n = S.utm_from_lonlat(lat, lon, GEOREF.epsg)
    u, v = (float(e) - GEOREF.ulx) / 10.0 - 0.5, (float(n) - GEOREF.uly) / -10.0 - 0.5
    assert c[20, 10, 0] == math.floor(u * 65536 + 0.5) and c[20, 10, 1] == math.floor(v * 65536 + 0.5)
    assert 40 < u < 70 and 30 < v < 70
    du = np.diff(c[..., 0].astype(np.int64), axis=1) / 65536
    assert abs(du.mean() - S.MERC_PIXEL / 10.0) < 0.01               # near the equator a grid pixel is 0.955 source pixels
    assert np.diff(c[..., 1].astype(np.int64), axis=0).min() > 0     # v grows southwards, as py does
    over = S.source_coords(S.Window(win.px0 - 96, win.py0 - 64, 128, 96), GEOREF)
    s = (over == S.INT32_MIN).all(axis=-1)
    assert ((over == S.INT32_MIN).any(axis=-1) == s).all() and 0.3 < s.mean() < 0.9 and not s[-1, -1] and s[0, 0]
    inside = over[~s].astype(np.int64)
    assert inside[:, 0].min() >= -32768 and inside[:, 1].min() >= -32768
    assert inside[:, 0].max() < (GEOREF.cols << 16) - 32768 and inside[:, 1].max() < (GEOREF.rows << 16) - 32768


MTD = """<?xml version="1.0" encoding="UTF-8" standalone="no"?>
<{p}Level-1C_Tile_ID {ns}>
  <{p}General_Info><TILE_ID>S2A_OPER_MSI_L1C_TL_TEST</TILE_ID></{p}General_Info>
  <{p}Geometric_Info>
    <Tile_Geocoding metadataLevel="Brief">
      <HORIZONTAL_CS_NAME>WGS84 / UTM zone 31N</HORIZONTAL_CS_NAME>
      <HORIZONTAL_CS_CODE>EPSG:32631</HORIZONTAL_CS_CODE>
      <Size resolution="10"><NROWS>300</NROWS><NCOLS>400</NCOLS></Size>
      <Size resolution="20"><NROWS>150</NROWS><NCOLS>200</NCOLS></Size>
      <Size resolution="60"><NROWS>50</NROWS><NCOLS>67</NCOLS></Size>
      <Geoposition resolution="10"><ULX>799980</ULX><ULY>100020</ULY><XDIM>10</XDIM><YDIM>-10</YDIM></Geoposition>
      <Geoposition resolution="20"><ULX>799980</ULX><ULY>100020</ULY><XDIM>20</XDIM><YDIM>-20</YDIM></Geoposition>
    </Tile_Geocoding>
  </{p}Geometric_Info>
</{p}Level-1C_Tile_ID>
"""


@pytest.mark.parametrize("p,ns", [("", ""), ("n1:", 'xmlns:n1="https://psd-14.sentinel2.eo.esa.int/PSD/S2_PDI_Level-1C_Tile_Metadata.xsd"')])
def test_mtd_tl_parser_with_and_without_a_namespace(tmp_path, p, ns):
    f = tmp_path / "MTD_TL.xml"
    f.write_text(MTD.format(p=p, ns=ns))
    assert S.parse_mtd_tl(str(f)) == GEOREF
    f.write_text(MTD.format(p=p, ns=ns).replace('<Size resolution="10">', '<Size resolution="15">'))
    with pytest.raises(ValueError, match="NROWS"):
        S.parse_mtd_tl(str(f))
    f.write_text(MTD.format(p=p, ns=ns).replace("EPSG:32631", "EPSG:3857"))
    with pytest.raises(ValueError, match="epsg"):
        S.parse_mtd_tl(str(f))


def test_default_namespace_on_every_element(tmp_path):
    f = tmp_path / "MTD_TL.xml"
    f.write_text(MTD.format(p="", ns='xmlns="urn:test"'))
    assert S.parse_mtd_tl(str(f)) == GEOREF


def test_sidecar_parser_and_find_product(tmp_path):
    side = tmp_path / "a.json"
    side.write_text(json.dumps(GEOREF._asdict()))
    assert S.read_sidecar(str(side)) == GEOREF
    (tmp_path / "a.tif").write_bytes(b"")
    assert S.find_product(str(tmp_path / "a.tif")) == (str(tmp_path / "a.tif"), GEOREF)
    (tmp_path / "b.png").write_bytes(b"")
    with pytest.raises(ValueError, match="sidecar b.json"):
        S.find_product(str(tmp_path / "b.png"))
    d = GEOREF._asdict()
    del d["ydim"]
    side.write_text(json.dumps(d))
    with pytest.raises(ValueError, match="ydim"):
        S.read_sidecar(str(side))
    for key, bad in (("ydim", 10.0), ("xdim", 0.0), ("rows", 0), ("cols", 40000), ("epsg", 3857)):
        side.write_text(json.dumps(dict(GEOREF._asdict(), **{key: bad})))
        with pytest.raises(ValueError, match="a.json"):
            S.read_sidecar(str(side))
    safe = tmp_path / "S2A_TEST.SAFE" / "GRANULE" / "L1C_T31NGA"
    (safe / "IMG_DATA").mkdir(parents=True)
    (safe / "IMG_DATA" / "T31NGA_20200101T000000_TCI.jp2").write_bytes(b"")
    (safe / "MTD_TL.xml").write_text(MTD.format(p="", ns=""))
    raster, g = S.find_product(str(tmp_path / "S2A_TEST.SAFE"))
    assert raster.endswith("_TCI.jp2") and g == GEOREF
    assert [p.rsplit("/", 1)[1] for p in S.list_products(str(tmp_path))] == ["S2A_TEST.SAFE", "a.tif", "b.png"]


@pytest.mark.parametrize("shift", [(500.0, -400.0), (-200.0, 150.0), (3500.0, -2600.0), (50000.0, 0.0)])
def test_the_crop_covers_every_coordinate_of_its_window(shift):
    """inside the raster, over its upper-left corner, over its lower-right corner, and a window that misses it"""
    win = _window_at(GEOREF.ulx + shift[0], GEOREF.uly + shift[1], GEOREF.epsg, 96, 64)
    c = S.source_coords(win, GEOREF).astype(np.int64)
    live = ~(c == S.INT32_MIN).all(axis=-1)
    box = S.source_crop(win, GEOREF)
    if shift[0] == 50000.0:
        assert box is None and not live.any()
        return
    x0, y0, x1, y1 = box
    assert 0 <= x0 < x1 <= GEOREF.cols and 0 <= y0 < y1 <= GEOREF.rows and live.any()
    xs, ys = c[..., 0][live] >> 16, c[..., 1][live] >> 16
    for lo, hi, vals, size in ((x0, x1, xs, GEOREF.cols), (y0, y1, ys, GEOREF.rows)):
        near, far = np.clip(vals, 0, size - 1), np.clip(vals + 1, 0, size - 1)
        assert near.min() >= lo and far.max() < hi
        assert lo == 0 or near.min() - lo >= 2                        # the pad, wherever the raster goes on
        assert hi == size or hi - 1 - far.max() >= 2
    assert (x1 - x0) * (y1 - y0) < 0.2 * GEOREF.rows * GEOREF.cols
    # the crop with its own georeference gives the window's pixels: at most one fixed-point unit of the shifted origin's rounding
    g2 = S.crop_georef(GEOREF, box)
    assert (g2.rows, g2.cols) == (y1 - y0, x1 - x0) and g2.ulx == GEOREF.ulx + 10.0 * x0 and g2.uly == GEOREF.uly - 10.0 * y0
    c2 = S.source_coords(win, g2).astype(np.int64)
    assert np.array_equal(~(c2 == S.INT32_MIN).all(axis=-1), live)
    assert np.abs(c2[live] + np.array([x0 << 16, y0 << 16]) - c[live]).max() <= 1
    src = np.random.RandomState(5).randint(0, 256, size=(1, GEOREF.rows, GEOREF.cols, 3)).astype(np.uint8)
    full, cropped = S.warp_bilinear(src, c.astype(np.int32)), S.warp_bilinear(src[:, y0:y1, x0:x1], c2.astype(np.int32))
    assert np.abs(full.astype(int) - cropped.astype(int)).max() <= 1 and (full != cropped).mean() < 0.01


def test_reproject_reference_stacks_the_frames():
    win = _window_at(GEOREF.ulx + 500.0, GEOREF.uly - 400.0, GEOREF.epsg, 32, 32)
    rng = np.random.RandomState(6)
    a, b = (rng.randint(0, 256, size=(GEOREF.rows, GEOREF.cols, 3)).astype(np.uint8) for _ in range(2))
    g20 = GEOREF._replace(xdim=20.0, ydim=-20.0)
    out = S.reproject_reference([a, b], [GEOREF, g20], win, "propagate")
    assert out.shape == (2, 32, 32, 3)
    assert np.array_equal(out[0], S.warp_bilinear(a[None], S.source_coords(win, GEOREF), "propagate")[0])
    assert np.array_equal(out[1], S.warp_bilinear(b[None], S.source_coords(win, g20), "propagate")[0])


# ---------------------------------------------------------------- 5. the driver's host side
def test_source_option_refusals_and_scene_listing(tmp_path):
    from satlas_super_resolution_amd.infer_scene import check_source, list_product_scenes
    assert check_source(None) is None and check_source(None, ["tci", "b08"]) is None      # absent: nothing new, s2_bands as ever
    assert check_source("sentinel2_l1c") == "sentinel2_l1c"
    with pytest.raises(ValueError, match="source"):
        check_source("sentinel2_l2a")
    with pytest.raises(ValueError, match="s2_bands"):
        check_source("sentinel2_l1c", ["tci", "b08"])
    (tmp_path / "b" / "S2B_X.SAFE").mkdir(parents=True)
    (tmp_path / "b" / "a.tif").write_bytes(b"")
    (tmp_path / "b" / "a.json").write_text("{}")
    (tmp_path / "a").mkdir()
    (tmp_path / "a" / "z.npy").write_bytes(b"")
    (tmp_path / "empty").mkdir()
    (tmp_path / "loose.png").write_bytes(b"")
    got = list_product_scenes(str(tmp_path))
    assert [(n, [p.rsplit("/", 1)[1] for p in ps]) for n, ps in got] == [("a", ["z.npy"]), ("b", ["S2B_X.SAFE", "a.tif"])]


def test_raster_crop_reader_and_the_local_pixel_limit(tmp_path):
    from PIL import Image
    from satlas_super_resolution_amd import png_io
    rng = np.random.RandomState(7)
    rgb = rng.randint(0, 256, size=(40, 50, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(tmp_path / "a.jp2", irreversible=False)
    Image.fromarray(rgb).save(tmp_path / "a.tif")
    Image.fromarray(rgb[..., 0]).save(tmp_path / "g.png")
    np.save(tmp_path / "a.npy", rgb)
    Image.fromarray(rgb.astype(np.uint16)[..., 0] * 200).save(tmp_path / "b16.png")
    before = Image.MAX_IMAGE_PIXELS
    for name in ("a.jp2", "a.tif", "a.npy"):
        assert png_io.raster_size(str(tmp_path / name)) == (40, 50)
        assert np.array_equal(png_io.read_raster_crop(str(tmp_path / name), (3, 5, 47, 40)), rgb[5:40, 3:47]), name
    assert np.array_equal(png_io.read_raster_crop(str(tmp_path / "g.png"), (0, 0, 50, 40)), np.repeat(rgb[..., :1], 3, axis=2))
    with pytest.raises(ValueError, match="16-bit"):
        png_io.read_raster_crop(str(tmp_path / "b16.png"), (0, 0, 50, 40))
    assert Image.MAX_IMAGE_PIXELS == before                          # raised inside the calls only, also when one raises
    with png_io._pixel_limit():
        assert Image.MAX_IMAGE_PIXELS >= 10980 * 10980
    assert Image.MAX_IMAGE_PIXELS == before
    assert set(png_io.raster_decoders()) == {"jpg_2000", "libtiff"}
    blk = png_io.ShmBlock(3 * 10 * 20 + 5, str(tmp_path), "t")
    try:
        assert png_io.read_crop_into(str(tmp_path / "a.tif"), (10, 20, 30, 30), blk.path, blk.nbytes, 5, True) == (10, 20, 3)
        assert np.array_equal(blk.buf[5:].reshape(10, 20, 3), rgb[20:30, 10:30]) and not blk.buf[:5].any()
    finally:
        blk.close()
