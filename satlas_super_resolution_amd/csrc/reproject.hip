// Raw Sentinel-2 L1C onto the model's grid (satlas_super_resolution_amd/s2_reproject.py states every formula; infer_scene.py drives):
// the source coordinates of every pixel centre of a window of the Web-Mercator grid in a UTM raster, and the integer bilinear warp
// that reads them.
//
//   merc_to_utm_coords_kernel     ssr_merc_to_utm_coords: one thread per output pixel, the whole chain in fp64 - global pixel centre
//                                 -> Mercator metres -> latitude (sinh, atan) and longitude -> transverse Mercator by the Krueger
//                                 series through n^6 (atanh, sinh, atan2, asinh, six sin / cos / sinh / cosh terms) -> source pixel
//                                 coordinates in 16.16 fixed point or the sentinel; one 8-byte store per thread, coalesced.  The
//                                 series' constants are computed on the host (utm_series) and passed by value.
//   scene_warp_bilinear_kernel<C> ssr_scene_warp_bilinear: one thread per (frame, output pixel); byte loads (no alignment of the
//                                 source is assumed: odd sizes and C = 3 give unaligned rows), 64-bit integer weights, the pixel's C
//                                 bytes written by its thread.  No atomics: a second launch writes the same bytes.
#include "common.h"

#include <cmath>

namespace {

constexpr double EARTH_R = 6378137.0;
constexpr double WGS84_F = 1.0 / 298.257223563;
constexpr double UTM_K0 = 0.9996;
constexpr double PI = 3.14159265358979323846;
constexpr int32_t SENTINEL = INT32_MIN;
constexpr int MAX_WINDOW = 4096;       // pixels per side of a window
constexpr int MAX_RASTER = 32767;      // rows / cols of a source raster: its coordinates fit the 16.16 words

struct UtmSeries {
    double e, k0A, lon0, fn;           // first eccentricity, k0 x rectifying radius, central meridian (radians), false northing
    double alpha[6];
};

struct CoordArgs {
    double px0, py0;                   // the window's first pixel centre, in global pixels
    double pixel, half;                // MERC_PIXEL, pi R
    double ulx, uly, xdim, ydim, rows, cols;
    int w, h;
};

UtmSeries utm_series(int zone, bool south) {
    UtmSeries s;
    const double f = WGS84_F, n = f / (2.0 - f), n2 = n * n;
    s.e = std::sqrt(f * (2.0 - f));
    s.k0A = UTM_K0 * (EARTH_R / (1.0 + n) * (1.0 + n2 / 4.0 + n2 * n2 / 64.0 + n2 * n2 * n2 / 256.0));
    s.lon0 = (6.0 * zone - 183.0) * (PI / 180.0);
    s.fn = south ? 10000000.0 : 0.0;
    // Karney 2011, eq. 35
    s.alpha[0] = n * (1.0 / 2 + n * (-2.0 / 3 + n * (5.0 / 16 + n * (41.0 / 180 + n * (-127.0 / 288 + n * (7891.0 / 37800))))));
    s.alpha[1] = n2 * (13.0 / 48 + n * (-3.0 / 5 + n * (557.0 / 1440 + n * (281.0 / 630 + n * (-1983433.0 / 1935360)))));
    s.alpha[2] = n2 * n * (61.0 / 240 + n * (-103.0 / 140 + n * (15061.0 / 26880 + n * (167603.0 / 181440))));
    s.alpha[3] = n2 * n2 * (49561.0 / 161280 + n * (-179.0 / 168 + n * (6601661.0 / 7257600)));
    s.alpha[4] = n2 * n2 * n * (34729.0 / 80640 + n * (-3418889.0 / 1995840));
    s.alpha[5] = n2 * n2 * n2 * (212378941.0 / 319334400);
    return s;
}

__global__ __launch_bounds__(256) void merc_to_utm_coords_kernel(CoordArgs a, UtmSeries s, int2* __restrict__ coords) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.w * a.h) return;
    const int row = (int)(i / a.w), col = (int)(i - (long)row * a.w);
    const double x = (a.px0 + col) * a.pixel - a.half, y = a.half - (a.py0 + row) * a.pixel;
    // the statement goes through degrees (merc_pixel_to_lonlat -> utm_from_lonlat); radians all the way here
    const double lam = x / EARTH_R - s.lon0, phi = atan(sinh(y / EARTH_R));
    const double tau = tan(phi), t1 = sqrt(1.0 + tau * tau);
    const double sigma = sinh(s.e * atanh(s.e * tau / t1));
    const double taup = tau * sqrt(1.0 + sigma * sigma) - sigma * t1;
    const double cl = cos(lam);
    const double xi0 = atan2(taup, cl), eta0 = asinh(sin(lam) / sqrt(taup * taup + cl * cl));
    double xi = xi0, eta = eta0;
#pragma unroll
    for (int j = 1; j <= 6; ++j) {
        const double ax = 2.0 * j * xi0, ae = 2.0 * j * eta0;
        xi += s.alpha[j - 1] * sin(ax) * cosh(ae);
        eta += s.alpha[j - 1] * cos(ax) * sinh(ae);
    }
    const double E = 500000.0 + s.k0A * eta, N = s.fn + s.k0A * xi;
    const double u = (E - a.ulx) / a.xdim - 0.5, v = (N - a.uly) / a.ydim - 0.5;
    int2 out = make_int2(SENTINEL, SENTINEL);
    if (u >= -0.5 && u < a.cols - 0.5 && v >= -0.5 && v < a.rows - 0.5)      // (a NaN fails every comparison: sentinel)
        out = make_int2((int)floor(u * 65536.0 + 0.5), (int)floor(v * 65536.0 + 0.5));
    coords[i] = out;
}

template <int C>
__global__ __launch_bounds__(256) void scene_warp_bilinear_kernel(const uint8_t* __restrict__ src, int Hs, int Ws,
                                                                  const int2* __restrict__ coords, long npix, int propagate,
                                                                  uint8_t* __restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const long t = blockIdx.y;
    uint8_t* o = dst + (t * npix + i) * C;
    const int2 c = coords[i];
    if (c.x == SENTINEL && c.y == SENTINEL) {
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = 0;
        return;
    }
    const int x0 = c.x >> 16, y0 = c.y >> 16;                  // arithmetic shifts: floor
    const uint64_t fx = (uint32_t)c.x & 0xffffu, fy = (uint32_t)c.y & 0xffffu;
    const int xa = min(max(x0, 0), Ws - 1), xb = min(max(x0 + 1, 0), Ws - 1);      // (x0 + 1 cannot overflow: x0 < 2^15)
    const int ya = min(max(y0, 0), Hs - 1), yb = min(max(y0 + 1, 0), Hs - 1);
    const uint8_t* f = src + t * Hs * (long)Ws * C;
    const uint8_t* p[4] = {f + ((long)ya * Ws + xa) * C, f + ((long)ya * Ws + xb) * C, f + ((long)yb * Ws + xa) * C,
                           f + ((long)yb * Ws + xb) * C};
    const uint64_t wgt[4] = {(65536 - fx) * (65536 - fy), fx * (65536 - fy), (65536 - fx) * fy, fx * fy};
    uint64_t acc[C];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = 1ull << 31;
    bool dead = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bool zero = false;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const uint32_t s = p[q][k];
            zero |= s == 0;
            acc[k] += wgt[q] * s;
        }
        dead |= zero && wgt[q] != 0;
    }
    if (propagate && dead) {
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) o[k] = (uint8_t)(acc[k] >> 32);
}

#define ST(s) reinterpret_cast<hipStream_t>(s)

}  // namespace

extern "C" int ssr_merc_to_utm_coords(int32_t px0, int32_t py0, int32_t w, int32_t h, int32_t epsg, double ulx, double uly,
                                      double xdim, double ydim, int32_t rows, int32_t cols, int32_t* coords, void* stream) {
    if (!coords || (reinterpret_cast<uintptr_t>(coords) & 7) || w <= 0 || h <= 0 || rows <= 0 || cols <= 0 || px0 < 0 || py0 < 0)
        return SSR_EINVAL;
    if (!(xdim > 0.0) || !(ydim < 0.0) || !std::isfinite(ulx) || !std::isfinite(uly) || !std::isfinite(xdim) || !std::isfinite(ydim))
        return SSR_EINVAL;
    const bool north = epsg >= 32601 && epsg <= 32660, south = epsg >= 32701 && epsg <= 32760;
    if (!(north || south) || w > MAX_WINDOW || h > MAX_WINDOW || rows > MAX_RASTER || cols > MAX_RASTER) return SSR_EUNSUP;
    if ((long)px0 + w > (1l << 22) || (long)py0 + h > (1l << 22)) return SSR_EINVAL;
    CoordArgs a;
    a.px0 = px0 + 0.5, a.py0 = py0 + 0.5;
    a.pixel = 2.0 * PI * EARTH_R / 4194304.0, a.half = PI * EARTH_R;
    a.ulx = ulx, a.uly = uly, a.xdim = xdim, a.ydim = ydim, a.rows = rows, a.cols = cols;
    a.w = w, a.h = h;
    const UtmSeries s = utm_series(epsg % 100, south);
    const long n = (long)w * h;
    hipLaunchKernelGGL(merc_to_utm_coords_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ST(stream), a, s,
                       reinterpret_cast<int2*>(coords));
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_warp_bilinear(const uint8_t* src, int32_t T, int32_t Hs, int32_t Ws, int32_t C, const int32_t* coords,
                                       int32_t h, int32_t w, int32_t mode, uint8_t* dst, void* stream) {
    if (!src || !coords || !dst || (reinterpret_cast<uintptr_t>(coords) & 7) || T <= 0 || Hs <= 0 || Ws <= 0 || h <= 0 || w <= 0 ||
        (mode != 0 && mode != 1))
        return SSR_EINVAL;
    if ((C != 1 && C != 3) || w > MAX_WINDOW || h > MAX_WINDOW || Hs > MAX_RASTER || Ws > MAX_RASTER || T > 65535) return SSR_EUNSUP;
    const long npix = (long)h * w;
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)T);
    const auto kernel = C == 3 ? scene_warp_bilinear_kernel<3> : scene_warp_bilinear_kernel<1>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ST(stream), src, Hs, Ws, reinterpret_cast<const int2*>(coords), npix, mode, dst);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
