// The convolution and pooling geometries of LPIPS's AlexNet backbone (lpips_metric.py, lpips_model 'alexnet') that lie outside
// ssr_conv2d's families (3x3 s1, 4x4 s2, 2x2 s1): an 11x11 stride-4 layer, a 5x5 layer and overlapping 3x3 stride-2 max pooling.
//
//   ssr_conv_direct      exact-fp32 direct (im2col-free) convolution, square odd kernels up to 11, stride 1..4, any grid
//   ssr_maxpool3s2_fwd   max pooling 3x3 stride 2 without padding (floor mode), optional ReLU
//
// ssr_conv_direct is an implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns 32 consecutive output pixels of ONE
// output row of ONE image and up to 128 output channels: wave w the 32 channels [128 ct + 32 w, + 32).  Per tap row ky and chunk
// of CC input channels the input row piece those 32 outputs read ((32 - 1) stride + K columns, zeros outside the image) is staged
// through LDS as [channel][column]; the A operand of lane (i, g) is patch[2 c2 + g][i stride + kx] (stride-1 layers: conflict-free,
// consecutive lanes read consecutive words), the B operand w[ky K + kx][c0 + 2 c2 + g][co0 + i] comes straight from the packed
// array (32 consecutive floats per half-wave).  Every output has ONE accumulator chain in the order ky, kx, c ascending; there is
// no split of K and no atomic, so two launches give the same bytes, and because a workgroup never holds pixels of two images an
// image's bytes do not depend on the batch.  Tap rows that lie wholly in the padding are skipped (they
// would add products with zero).  Validation-only work: measured once, not tuned (profiles/lpips_alex).
#include "common.h"

namespace {

constexpr int CD_TP = 32;                                   // output pixels (of one row) per workgroup
constexpr int CD_MAXK = 11, CD_MAXS = 4;
constexpr int CD_COLS = (CD_TP - 1) * CD_MAXS + CD_MAXK;   // 135: input columns a workgroup reads at the most
constexpr int CD_PITCH = 137;                               // LDS row pitch in words (odd: the two lane halves land on different banks)
constexpr int CD_CO = 128;                                  // output channels per workgroup

struct cd_args {
    ssr_view x, y;
    const float* w;
    const float* bias;
    int Hi, Wi, Cin, Cout, K, stride, pad, Ho, Wo, relu;
    int xt, ct;                                             // pixel tiles per output row, channel tiles
};

// grid: one workgroup per (image, output row, pixel tile, channel tile), channel tile fastest
template <int CC>
__global__ __launch_bounds__(256) void conv_direct_kernel(cd_args a) {
    __shared__ float patch[CC * CD_PITCH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, g = lane >> 5;
    long b = blockIdx.x;
    const int ct = (int)(b % a.ct); b /= a.ct;
    const int xt = (int)(b % a.xt); b /= a.xt;
    const int oy = (int)(b % a.Ho);
    const long n = b / a.Ho;
    const int co0 = ct * CD_CO + wave * 32;
    const bool live = co0 < a.Cout;                         // wave-uniform; an idle wave still stages and meets the barriers
    const int ox0 = xt * CD_TP;
    const int ix0 = ox0 * a.stride - a.pad;
    const int ncols = (CD_TP - 1) * a.stride + a.K;         // <= CD_COLS
    const float* __restrict__ xp = reinterpret_cast<const float*>(a.x.p) + a.x.coff;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int ky = 0; ky < a.K; ++ky) {
        const int iy = oy * a.stride - a.pad + ky;
        if (iy < 0 || iy >= a.Hi) continue;                 // workgroup-uniform
        const long rowbase = (n * a.Hi + iy) * a.Wi;
        for (int c0 = 0; c0 < a.Cin; c0 += CC) {
            __syncthreads();                                // the previous chunk has been read
            for (int t = threadIdx.x; t < ncols * (CC / 4); t += 256) {
                const int col = t / (CC / 4), q = t % (CC / 4);
                const int ix = ix0 + col;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (ix >= 0 && ix < a.Wi) v = *reinterpret_cast<const f32x4*>(xp + (rowbase + ix) * a.x.cs + c0 + 4 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) patch[(4 * q + k) * CD_PITCH + col] = v[k];
            }
            __syncthreads();
            if (live) {
                const float* arow = patch + g * CD_PITCH + i * a.stride;
                for (int kx = 0; kx < a.K; ++kx) {
                    const float* __restrict__ wp = a.w + ((long)(ky * a.K + kx) * a.Cin + c0 + g) * a.Cout + co0 + i;
#pragma unroll
                    for (int c2 = 0; c2 < CC / 2; ++c2)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * c2 * CD_PITCH + kx], wp[(long)(2 * c2) * a.Cout], acc, 0, 0, 0);
                }
            }
        }
    }
    if (!live) return;
    const float bb = a.bias ? a.bias[co0 + i] : 0.f;
    float* __restrict__ yp = reinterpret_cast<float*>(a.y.p) + a.y.coff + co0 + i;
    const long orow = (n * a.Ho + oy) * a.Wo;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ox = ox0 + mfma32_row(r, g);
        if (ox < a.Wo) {
            float v = acc[r] + bb;
            if (a.relu) v = v < 0.f ? 0.f : v;              // (a NaN stays a NaN)
            yp[(orow + ox) * a.y.cs] = v;
        }
    }
}

// one thread: four channels of one output pixel
__global__ __launch_bounds__(256) void maxpool3s2_kernel(ssr_view f, ssr_view p, int H, int W, int Ho, int Wo, int C4, long total, int relu) {
    const float* __restrict__ fp = reinterpret_cast<const float*>(f.p) + f.coff;
    float* __restrict__ pp = reinterpret_cast<float*>(p.p) + p.coff;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % C4);
        long t = e / C4;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const long n = t / Ho;
        const long base = (n * H + 2 * oy) * W + 2 * ox;
        f32x4 m = *reinterpret_cast<const f32x4*>(fp + base * f.cs + 4 * c4);
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const f32x4 v = *reinterpret_cast<const f32x4*>(fp + (base + (long)dy * W + dx) * f.cs + 4 * c4);
#pragma unroll
                for (int k = 0; k < 4; ++k) m[k] = (v[k] > m[k] || v[k] != v[k]) ? v[k] : m[k];      // a NaN wins, as in torch
            }
        if (relu) {       // max(0, .) is monotone: applied to the maximum it gives what applying it to the nine values first gives
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = m[k] < 0.f ? 0.f : m[k];
        }
        *reinterpret_cast<f32x4*>(pp + ((n * Ho + oy) * Wo + ox) * p.cs + 4 * c4) = m;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool view_aligned(const ssr_view& v) { return v.coff >= 0 && (v.cs % 4) == 0 && (v.coff % 4) == 0 && aligned16(v.p); }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_conv_direct(ssr_view x, ssr_view y, const float* w, const float* bias, int32_t dtype, int32_t N, int32_t Hi,
                               int32_t Wi, int32_t Cin, int32_t Cout, int32_t K, int32_t stride, int32_t pad, int32_t relu,
                               void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32) return SSR_EUNSUP;
    if (!x.p || !y.p || !w || N <= 0 || Hi <= 0 || Wi <= 0 || Cin <= 0 || Cout <= 0 || K <= 0 || stride <= 0 || pad < 0) return SSR_EINVAL;
    if ((K % 2) == 0 || K > CD_MAXK || stride > CD_MAXS || pad > K / 2) return SSR_EUNSUP;
    if ((Cin % 8) || Cin > 512 || (Cout % 32) || Cout > 512) return SSR_EUNSUP;
    if (Hi + 2 * pad < K || Wi + 2 * pad < K) return SSR_EINVAL;                   // no output pixel
    if (x.coff < 0 || y.coff < 0 || x.cs < x.coff + Cin || y.cs < y.coff + Cout) return SSR_EINVAL;
    if (!view_aligned(x) || !view_aligned(y) || !aligned16(w) || (reinterpret_cast<uintptr_t>(bias) & 3)) return SSR_EINVAL;
    cd_args a;
    a.x = x; a.y = y; a.w = w; a.bias = bias;
    a.Hi = Hi; a.Wi = Wi; a.Cin = Cin; a.Cout = Cout; a.K = K; a.stride = stride; a.pad = pad; a.relu = relu ? 1 : 0;
    a.Ho = (Hi + 2 * pad - K) / stride + 1;
    a.Wo = (Wi + 2 * pad - K) / stride + 1;
    a.xt = (a.Wo + CD_TP - 1) / CD_TP;
    a.ct = (Cout + CD_CO - 1) / CD_CO;
    const long blocks = (long)N * a.Ho * a.xt * a.ct;
    if (blocks > 0x7fffffffL) return SSR_EINVAL;
    if (Cin % 32 == 0) hipLaunchKernelGGL(conv_direct_kernel<32>, dim3((unsigned)blocks), dim3(256), 0, ST(stream), a);
    else hipLaunchKernelGGL(conv_direct_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, ST(stream), a);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_maxpool3s2_fwd(ssr_view f, ssr_view p, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t relu,
                                  void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32) return SSR_EUNSUP;
    if (!f.p || !p.p || N <= 0 || H < 3 || W < 3 || C <= 0) return SSR_EINVAL;
    if (C % 4) return SSR_EUNSUP;
    if (f.coff < 0 || p.coff < 0 || f.cs < f.coff + C || p.cs < p.coff + C || !view_aligned(f) || !view_aligned(p)) return SSR_EINVAL;
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1, C4 = C / 4;
    const long total = (long)N * Ho * Wo * C4;
    long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3((int)g), dim3(256), 0, ST(stream), f, p, (int)H, (int)W, Ho, Wo, C4, total, relu ? 1 : 0);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
