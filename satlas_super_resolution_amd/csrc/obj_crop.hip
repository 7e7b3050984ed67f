// Crop-and-resize of the OpenStreetMap object boxes, forward and backward (include/ssr_hip.h, ssr_obj_crop_resize_fwd / _bwd).
//
// Replaces the device work of the reference model's per-object loop (ssr/models/osm_objs_esrgan_model.py:166-181: slice a box out of
// an image, torchvision resize to 32 x 32, bilinear, align_corners = False, with or without antialiasing) and of autograd's backward
// of it.  The boxes are DATA: both kernels read them from device memory, so a captured graph replays with the next step's boxes.
//
// The work is tiny - Bo * 1024 * 3 outputs of at most 64 taps each - so both kernels are bound by launch and latency.
// Forward : one workgroup per crop.  64 threads build the two tap tables (first tap, tap count, <= 8 normalised weights per output
//           row / column) in LDS; then every thread owns 4 output pixels, reads its taps as one 16-byte load per source pixel where
//           the view allows it, and writes its pixel's 8 channels (3 values, 5 zeros) as two 16-byte stores.
// Backward: the gather form.  One workgroup per 16 x 16 tile of one image; it walks the image's objects in index order (first[b] ..
//           first[b + 1]), skips the ones its tile does not touch (a uniform branch), rebuilds the object's tap tables in LDS and lets
//           every covered pixel sum, in (oy, ox) order, over the outputs whose taps reach it.  One writer per image pixel, no atomics:
//           two runs give the same bytes; a pixel no box covers is not written at all.
// Both directions sum one axis first (x, then y): the 2-D weight is the product of the two axes' weights, and the backward is the
// forward's transpose.
#include "common.h"

namespace {

constexpr int OC_OUT = SSR_OBJ_CROP;          // 32: side of a resized crop
constexpr int OC_TAPS = 8;                    // taps per axis at SSR_OBJ_MAX_SIDE -> 32 with antialiasing (floor(2 * scale) + 1, scale <= 4)
constexpr int OC_NT = 256;
constexpr int OC_TILE = 16;                   // backward: image tile side (OC_TILE * OC_TILE == OC_NT)

struct Taps {
    int first[2][OC_OUT];                     // [axis: 0 = x, 1 = y][output index]
    int count[2][OC_OUT];
    float w[2][OC_OUT][OC_TAPS];
};

// The tap rule of the resize for output i of an axis of n_in source pixels (n_in <= SSR_OBJ_MAX_SIDE).  scale = n_in / 32, center and
// both bounds are exact in fp32 at these sizes (7-bit by 6-bit products); the weights carry a few ulps of rounding.
__device__ __forceinline__ void build_taps(int n_in, int i, bool antialias, int& first, int& count, float* w) {
    const float scale = (float)n_in / (float)OC_OUT;
    const float support = (antialias && scale >= 1.f) ? scale : 1.f;
    const float center = scale * ((float)i + 0.5f);
    int lo = (int)(center - support + 0.5f);
    lo = lo < 0 ? 0 : lo;
    int hi = (int)(center + support + 0.5f);
    hi = hi > n_in ? n_in : hi;
    int n = hi - lo;
    n = n < 0 ? 0 : (n > OC_TAPS ? OC_TAPS : n);
    float total = 0.f;
#pragma unroll
    for (int j = 0; j < OC_TAPS; ++j) {
        float v = 0.f;
        if (j < n) {
            v = 1.f - fabsf(((float)(j + lo) - center + 0.5f) / support);
            v = v < 0.f ? 0.f : v;
        }
        w[j] = v;
        total += v;
    }
#pragma unroll
    for (int j = 0; j < OC_TAPS; ++j) w[j] = total > 0.f ? w[j] / total : 0.f;
    first = lo;
    count = n;
}

struct Box { int b, x1, y1, x2, y2; bool ok; };

// A box is served when it lies inside image b of [B, H, W], is not empty and has no side above SSR_OBJ_MAX_SIDE; every other box is
// refused: zero crop, no gradient, nothing read through it.
__device__ __forceinline__ Box load_box(const int32_t* boxes, int o, int B, int H, int W) {
    Box q;
    q.b = boxes[5 * o + 0]; q.x1 = boxes[5 * o + 1]; q.y1 = boxes[5 * o + 2]; q.x2 = boxes[5 * o + 3]; q.y2 = boxes[5 * o + 4];
    q.ok = q.b >= 0 && q.b < B && q.x1 >= 0 && q.y1 >= 0 && q.x2 > q.x1 && q.y2 > q.y1 && q.x2 <= W && q.y2 <= H &&
           q.x2 - q.x1 <= SSR_OBJ_MAX_SIDE && q.y2 - q.y1 <= SSR_OBJ_MAX_SIDE;
    return q;
}

__device__ __forceinline__ void fill_taps(Taps& T, const Box& q, bool antialias) {
    const int t = threadIdx.x;
    if (t < 2 * OC_OUT) {
        const int axis = t / OC_OUT, i = t % OC_OUT;
        build_taps(axis == 0 ? q.x2 - q.x1 : q.y2 - q.y1, i, antialias, T.first[axis][i], T.count[axis][i], T.w[axis][i]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(OC_NT) void obj_crop_fwd_kernel(ssr_view src, int B, int H, int W, const int32_t* __restrict__ boxes,
                                                             ssr_view dst, int antialias) {
    __shared__ Taps T;
    const int o = blockIdx.x;
    const Box q = load_box(boxes, o, B, H, W);
    float* out = (float*)dst.p + (size_t)o * OC_OUT * OC_OUT * dst.cs + dst.coff;
    if (q.ok) fill_taps(T, q, antialias != 0);
    __syncthreads();
    const float* img = (const float*)src.p + src.coff;
    for (int p = threadIdx.x; p < OC_OUT * OC_OUT; p += OC_NT) {
        const int oy = p / OC_OUT, ox = p % OC_OUT;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (q.ok) {
            const int ny = T.count[1][oy], nx = T.count[0][ox];
            const int y0 = q.y1 + T.first[1][oy], x0 = q.x1 + T.first[0][ox];
            for (int ky = 0; ky < ny; ++ky) {
                const float wy = T.w[1][oy][ky];
                if (wy == 0.f) continue;           // zero-weight taps are skipped: an identity resize (32 x 32) returns the crop's own bits
                const float* row = img + ((size_t)q.b * H + (y0 + ky)) * W * src.cs;
                float r0 = 0.f, r1 = 0.f, r2 = 0.f;
                for (int kx = 0; kx < nx; ++kx) {
                    const float wx = T.w[0][ox][kx];
                    if (wx == 0.f) continue;
                    const float* px = row + (size_t)(x0 + kx) * src.cs;
                    float v0, v1, v2;
                    if constexpr (VEC) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(px);
                        v0 = v[0]; v1 = v[1]; v2 = v[2];
                    } else {
                        v0 = px[0]; v1 = px[1]; v2 = px[2];
                    }
                    r0 = fmaf(wx, v0, r0); r1 = fmaf(wx, v1, r1); r2 = fmaf(wx, v2, r2);
                }
                a0 = fmaf(wy, r0, a0); a1 = fmaf(wy, r1, a1); a2 = fmaf(wy, r2, a2);
            }
        }
        f32x4* d = reinterpret_cast<f32x4*>(out + (size_t)p * dst.cs);
        d[0] = f32x4{a0, a1, a2, 0.f};
        d[1] = f32x4{0.f, 0.f, 0.f, 0.f};       // channels 3..7: the first object convolution reads 8
    }
}

// outputs of one axis whose taps reach source position p: first[] and first[] + count[] are non-decreasing in the output index, so
// they form one contiguous range [lo, hi)
__device__ __forceinline__ void reach(const int* first, const int* count, int p, int& lo, int& hi) {
    lo = OC_OUT; hi = 0;
    for (int i = 0; i < OC_OUT; ++i) {
        const bool in = p >= first[i] && p < first[i] + count[i];
        if (in) { lo = i < lo ? i : lo; hi = i + 1; }
    }
}

__global__ __launch_bounds__(OC_NT) void obj_crop_bwd_kernel(ssr_view g, const int32_t* __restrict__ boxes,
                                                             const int32_t* __restrict__ first, int Bo, ssr_view dimg, int B, int H, int W,
                                                             float grad_scale, int antialias) {
    __shared__ Taps T;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * OC_TILE, tx0 = blockIdx.x * OC_TILE;
    const int y = ty0 + (int)threadIdx.x / OC_TILE, x = tx0 + (int)threadIdx.x % OC_TILE;
    int o0 = first[b], o1 = first[b + 1];
    o0 = o0 < 0 ? 0 : o0;
    o1 = o1 > Bo ? Bo : o1;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    bool covered = false;
    for (int o = o0; o < o1; ++o) {                                  // uniform over the workgroup
        const Box q = load_box(boxes, o, B, H, W);
        if (!q.ok || q.b != b) continue;
        if (q.x2 <= tx0 || q.x1 >= tx0 + OC_TILE || q.y2 <= ty0 || q.y1 >= ty0 + OC_TILE) continue;
        __syncthreads();                                             // the previous object's tables are no longer read
        fill_taps(T, q, antialias != 0);
        __syncthreads();
        if (x < q.x1 || x >= q.x2 || y < q.y1 || y >= q.y2) continue; // (no barrier below this line in the iteration)
        covered = true;
        int ylo, yhi, xlo, xhi;
        reach(T.first[1], T.count[1], y - q.y1, ylo, yhi);
        reach(T.first[0], T.count[0], x - q.x1, xlo, xhi);
        const float* go = (const float*)g.p + (size_t)o * OC_OUT * OC_OUT * g.cs + g.coff;
        for (int oy = ylo; oy < yhi; ++oy) {                          // a row's sum first: up to 32 x 32 terms reach one pixel of a tiny box
            const float wy = T.w[1][oy][y - q.y1 - T.first[1][oy]];
            float r0 = 0.f, r1 = 0.f, r2 = 0.f;
            for (int ox = xlo; ox < xhi; ++ox) {
                const float wx = T.w[0][ox][x - q.x1 - T.first[0][ox]];
                const float* gp = go + (size_t)(oy * OC_OUT + ox) * g.cs;
                r0 = fmaf(wx, gp[0], r0); r1 = fmaf(wx, gp[1], r1); r2 = fmaf(wx, gp[2], r2);
            }
            a0 = fmaf(wy, r0, a0); a1 = fmaf(wy, r1, a1); a2 = fmaf(wy, r2, a2);
        }
    }
    if (covered) {
        float* d = (float*)dimg.p + (((size_t)b * H + y) * W + x) * dimg.cs + dimg.coff;
        d[0] = fmaf(grad_scale, a0, d[0]); d[1] = fmaf(grad_scale, a1, d[1]); d[2] = fmaf(grad_scale, a2, d[2]);
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// fp32 storage only (SSR_F32 / SSR_F32X3), as the object branch itself
inline int oc_dtype(int32_t dtype) {
    if (dtype == SSR_F32 || dtype == SSR_F32X3) return SSR_OK;
    return dtype == SSR_BF16 ? SSR_EUNSUP : SSR_EINVAL;
}

// a [.., 32, 32, cs] view of crops whose 8 channels from coff are read / written as 16-byte pieces
inline bool oc_crop_view_ok(const ssr_view& v) { return v.p && al16(v.p) && v.cs > 0 && v.cs % 4 == 0 && v.coff >= 0 && v.coff % 4 == 0 && v.coff + 8 <= v.cs; }
inline bool oc_image_view_ok(const ssr_view& v) { return v.p && al4(v.p) && v.cs > 0 && v.coff >= 0 && v.coff + 3 <= v.cs; }

}  // namespace

extern "C" int ssr_obj_crop_resize_fwd(ssr_view src, int32_t dtype, int32_t B, int32_t H, int32_t W, const int32_t* boxes, int32_t Bo,
                                       ssr_view dst, int32_t antialias, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Bo <= 0 || !boxes || !al4(boxes) || !oc_image_view_ok(src) || !oc_crop_view_ok(dst)) return SSR_EINVAL;
    const int rc = oc_dtype(dtype);
    if (rc != SSR_OK) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool vec = al16(src.p) && src.cs % 4 == 0 && src.coff % 4 == 0 && src.coff + 4 <= src.cs;
    if (vec) hipLaunchKernelGGL(obj_crop_fwd_kernel<true>, dim3(Bo), dim3(OC_NT), 0, st, src, (int)B, (int)H, (int)W, boxes, dst, (int)antialias);
    else hipLaunchKernelGGL(obj_crop_fwd_kernel<false>, dim3(Bo), dim3(OC_NT), 0, st, src, (int)B, (int)H, (int)W, boxes, dst, (int)antialias);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_obj_crop_resize_bwd(ssr_view g, const int32_t* boxes, const int32_t* first, int32_t Bo, ssr_view dimg, int32_t dtype,
                                       int32_t B, int32_t H, int32_t W, float grad_scale, int32_t antialias, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Bo <= 0 || !boxes || !first || !al4(boxes) || !al4(first) || !oc_crop_view_ok(g) ||
        !oc_image_view_ok(dimg) || g.p == dimg.p)
        return SSR_EINVAL;
    const int rc = oc_dtype(dtype);
    if (rc != SSR_OK) return rc;
    const int gx = (W + OC_TILE - 1) / OC_TILE, gy = (H + OC_TILE - 1) / OC_TILE;
    if (gy > 65535 || B > 65535) return SSR_EUNSUP;
    hipLaunchKernelGGL(obj_crop_bwd_kernel, dim3(gx, gy, B), dim3(OC_NT), 0, reinterpret_cast<hipStream_t>(stream), g, boxes, first, (int)Bo,
                       dimg, (int)B, (int)H, (int)W, grad_scale, (int)antialias);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
