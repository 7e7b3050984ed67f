// LPIPS's own arithmetic (the `calculate_lpips` validation metric, /root/reference/ssr/metrics/lpips.py:7-21, lpips_model 'vgg'):
// the VGG16 convolutions run on the conv kernels in exact fp32 (SSR_ACT_RELU epilogue) and "ReLU + max-pool behind a tap" is
// ssr_relu_maxpool2_fwd (csrc/vgg.hip); what is left is HBM-bound NHWC glue.
//
//   ssr_lpips_input   uint8 [npix][3] -> the scaling layer's output, fp32 NHWC with 8-channel padding (3 valid channels, 5 zeros)
//   ssr_lpips_layer   one tap: per image the block partials of (1/HW) sum_p sum_c w[c] (a^ - b^)^2, a^ = a / (|a|_2 + 1e-10) per pixel
//
// ssr_lpips_layer is a row reduction over contiguous NHWC rows (256 B at C = 64, 2 KB at C = 512): 16 lanes share one pixel and
// read it as float4 (lane j: channels 64 i + 4 j .. + 3, i < C / 64: every load instruction of a wave covers four whole 256-byte
// pieces), keep both images' channels in registers between the norm pass and the difference pass (each feature is read once),
// and reduce across the 16 lanes with xor shuffles.  No atomics: one fp64 partial per block, added on the host in index order.
#include "common.h"

namespace {

struct lpips_in_args { float shift[3], scale[3]; int perm[3]; int normalize; };

// one thread: one pixel
__global__ __launch_bounds__(256) void lpips_input_kernel(const uint8_t* __restrict__ u, ssr_view y, long npix, lpips_in_args a) {
    float* __restrict__ yp = reinterpret_cast<float*>(y.p);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < npix; e += (long)gridDim.x * blockDim.x) {
        const uint8_t px[3] = {u[3 * e], u[3 * e + 1], u[3 * e + 2]};
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = (float)px[a.perm[c]] / 255.0f;          // IEEE division (correctly rounded), as numpy's
            if (a.normalize) v = 2.0f * v - 1.0f;             // 2 v is exact, so a fused multiply-add gives the same bits
            o[c] = (v - a.shift[c]) / a.scale[c];
        }
        float* dst = yp + e * y.cs + y.coff;
        *reinterpret_cast<f32x4*>(dst) = o;
        *reinterpret_cast<f32x4*>(dst + 4) = zero;
    }
}

__device__ __forceinline__ double group16_sum(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);        // butterfly: every lane of the group ends with the same bits
    return v;
}

// V = C / 64 float4 per lane and image.  grid (nblk, N), 256 threads = 16 pixel groups of 16 lanes.
template <int V>
__global__ __launch_bounds__(256) void lpips_layer_kernel(ssr_view fa, ssr_view fb, const float* __restrict__ w, int HW, int relu,
                                                          double* __restrict__ partial) {
// a^ - b^ is the difference of two ROUNDED products: a fused multiply-add would leave the rounding error of one of them behind
// for identical inputs, where the result has to be exactly 0
#pragma clang fp contract(off)
    const int n = blockIdx.y, lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const float* __restrict__ ap = reinterpret_cast<const float*>(fa.p) + fa.coff + 4 * lane;
    const float* __restrict__ bp = reinterpret_cast<const float*>(fb.p) + fb.coff + 4 * lane;
    f32x4 wv[V];
#pragma unroll
    for (int i = 0; i < V; ++i) wv[i] = *reinterpret_cast<const f32x4*>(w + 64 * i + 4 * lane);
    double acc = 0.0;
    // the trip count is the same for every thread of the block (the shuffles below need whole groups; a group past the end
    // works on zeros, which contribute 0 / (0 + 1e-10) = 0)
    for (int p0 = blockIdx.x * 16; p0 < HW; p0 += gridDim.x * 16) {
        const int p = p0 + grp;
        const bool ok = p < HW;
        const long row = (long)n * HW + p;
        f32x4 a[V], b[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            a[i] = ok ? *reinterpret_cast<const f32x4*>(ap + row * fa.cs + 64 * i) : zero;
            b[i] = ok ? *reinterpret_cast<const f32x4*>(bp + row * fb.cs + 64 * i) : zero;
        }
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (relu) { a[i][k] = fmaxf(a[i][k], 0.f); b[i][k] = fmaxf(b[i][k], 0.f); }
                sa += (double)a[i][k] * (double)a[i][k];      // exact products (24 x 24 bits), fp64 sums
                sb += (double)b[i][k] * (double)b[i][k];
            }
        const double ra = 1.0 / (sqrt(group16_sum(sa)) + 1e-10), rb = 1.0 / (sqrt(group16_sum(sb)) + 1e-10);
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = (float)((double)a[i][k] * ra - (double)b[i][k] * rb);     // the difference itself, in fp64
                acc += (double)(wv[i][k] * (d * d));                                       // fp32 products, fp64 sum
            }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long)n * gridDim.x + blockIdx.x] = (((red[0] + red[1]) + red[2]) + red[3]) / (double)HW;
}

inline int layer_blocks(long HW) {
    long b = (HW + 63) / 64;          // four rounds of 16 pixels per block, 256 blocks per image at the most
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

template <int V>
void launch_layer(ssr_view fa, ssr_view fb, const float* w, int N, int HW, int relu, double* partial, hipStream_t st) {
    hipLaunchKernelGGL(lpips_layer_kernel<V>, dim3(layer_blocks(HW), N), dim3(256), 0, st, fa, fb, w, HW, relu, partial);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_lpips_input(const uint8_t* u, ssr_view y, int32_t dtype, int64_t npix, const float* shift, const float* scale,
                               const int32_t* perm, int32_t normalize, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32) return SSR_EUNSUP;
    if (!u || !y.p || !shift || !scale || !perm || npix <= 0 || npix > (1ll << 40)) return SSR_EINVAL;
    if (y.coff < 0 || y.cs < y.coff + 8 || (y.cs % 4) || (y.coff % 4) || !aligned16(y.p)) return SSR_EINVAL;
    lpips_in_args a;
    for (int c = 0; c < 3; ++c) {
        if (perm[c] < 0 || perm[c] > 2 || !(scale[c] != 0.f)) return SSR_EINVAL;
        a.shift[c] = shift[c]; a.scale[c] = scale[c]; a.perm[c] = perm[c];
    }
    a.normalize = normalize ? 1 : 0;
    long g = (npix + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(lpips_input_kernel, dim3((int)g), dim3(256), 0, ST(stream), u, y, (long)npix, a);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_lpips_layer_blocks(int32_t N, int32_t HW, int32_t C) {
    if (N <= 0 || HW <= 0 || C <= 0) return SSR_EINVAL;
    return layer_blocks(HW);
}

extern "C" int ssr_lpips_layer(ssr_view fa, ssr_view fb, const float* w, int32_t dtype, int32_t N, int32_t HW, int32_t C,
                               int32_t relu, double* partial, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32) return SSR_EUNSUP;
    if (!fa.p || !fb.p || !w || !partial || N <= 0 || N > 65535 || HW <= 0 || C <= 0) return SSR_EINVAL;
    if (fa.coff < 0 || fb.coff < 0 || fa.cs < fa.coff + C || fb.cs < fb.coff + C) return SSR_EINVAL;
    if ((C % 64) || C > 512) return SSR_EUNSUP;
    if ((fa.cs % 4) || (fa.coff % 4) || (fb.cs % 4) || (fb.coff % 4) || !aligned16(fa.p) || !aligned16(fb.p) || !aligned16(w) ||
        (reinterpret_cast<uintptr_t>(partial) & 7))
        return SSR_EINVAL;
    const hipStream_t st = ST(stream);
    switch (C / 64) {
        case 1: launch_layer<1>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 2: launch_layer<2>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 3: launch_layer<3>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 4: launch_layer<4>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 5: launch_layer<5>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 6: launch_layer<6>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        case 7: launch_layer<7>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
        default: launch_layer<8>(fa, fb, w, N, HW, relu ? 1 : 0, partial, st); break;
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
