// The pixel and GAN losses of BasicSR 1.4.2 that ssr_l1_loss / ssr_bce_logits_loss (csrc/misc.hip) do not cover, each with its gradient
// in ONE launch (ssr_pixel_loss, ssr_gan_loss: include/ssr_hip.h; the CPU statement is satlas_super_resolution_amd/gan_pixel_losses.py):
//   basicsr/losses/basic_loss.py   MSELoss (mse_loss: F.mse_loss), CharbonnierLoss (charbonnier_loss: sqrt((pred - target)^2 + eps)),
//                                  reduction 'mean', times loss_weight
//   basicsr/losses/gan_loss.py     GANLoss.forward with gan_type lsgan (nn.MSELoss against the label map), wgan (_wgan_loss), wgan_softplus
//                                  (_wgan_softplus_loss) and hinge (nn.ReLU on 1 -+ input for the discriminator, -input.mean() for the
//                                  generator); get_target_label: only lsgan (and vanilla) read the label values
// A thread owns whole pixels: its address is one 64-bit multiply, the channels follow without a division; where the views allow it the
// C <= 4 channels of a pixel come in as one 16-byte (bf16: 8-byte) load.  The inputs
// are read once, the gradient is written in the same pass, nothing else is touched.  Terms are fp32 whatever the storage type; a
// thread's and a block's partial sums are kept in fp64 (the means of wgan / hinge cancel, an fp32 running sum would carry the
// rounding of its largest partial), the block's result is scaled and rounded to fp32 once.
#include "common.h"

namespace {

constexpr int NT = 256;           // threads of a block
constexpr int SPAN = 4 * NT;      // pixels per block the host sizes the grid with (as ssr_l1_loss: 256 * 4)
constexpr int CAP = 1024;         // blocks at most; SSR_LOSS_SLOTS under SSR_DETERMINISTIC

enum { PIX_MSE = 1, PIX_CHARBONNIER = 2 };
enum { GAN_LSGAN = 1, GAN_LINEAR = 2, GAN_SOFTPLUS = 3, GAN_HINGE_D = 4 };      // forms of the kernel (the host maps gan_type / is_disc)

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef f32x4 type; };
template <> struct Vec4<__bf16> { typedef bf16x4 type; };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// sum over the NT threads in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) s += sh[k];
    }
    return s;
}

// det: one slot per block, `+=` by the slot's single writer (launches on a stream are ordered) - the reader adds the slots in index
// order; default: one fp32 atomic per block (arrival order), as ssr_l1_loss
__device__ __forceinline__ void emit(float* __restrict__ out, float v, bool det) {
    if (det) out[blockIdx.x] += v; else atomicAdd(out, v);
}

template <int KIND> __device__ __forceinline__ void pixel_term(float d, float eps, float gscale, double& s, float& g) {
    if constexpr (KIND == PIX_MSE) {
        s += (double)(d * d);
        g = 2.f * gscale * d;
    } else {
        const float r = sqrtf(d * d + eps);
        s += (double)r;
        g = d == 0.f ? 0.f : gscale * d / r;      // eps == 0: 0 / 0 is 0 here, as the limit of every eps > 0
    }
}

// gscale = weight / (npix * C)
template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(NT) void pixel_loss_kernel(ssr_view a, ssr_view b, ssr_view grad, long npix, int C, float eps, float gscale,
                                                        float* __restrict__ loss_out, bool det) {
    __shared__ double sh[NT / 64];
    typedef typename Vec4<T>::type V;
    const T* __restrict__ ap = reinterpret_cast<const T*>(a.p) + a.coff;
    const T* __restrict__ bp = reinterpret_cast<const T*>(b.p) + b.coff;
    T* __restrict__ gp = grad.p ? reinterpret_cast<T*>(grad.p) + grad.coff : nullptr;
    double s = 0.0;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const T* __restrict__ pa = ap + p * a.cs;
        const T* __restrict__ pb = bp + p * b.cs;
        T* __restrict__ pg = gp ? gp + p * grad.cs : nullptr;
        if constexpr (VEC) {      // C <= 4 and both pixels are aligned groups of four inside their views (the host checked)
            const V va = *reinterpret_cast<const V*>(pa), vb = *reinterpret_cast<const V*>(pb);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    float g;
                    pixel_term<KIND>(to_f32(va[c]) - to_f32(vb[c]), eps, gscale, s, g);
                    if (pg) pg[c] = from_f32<T>(g);
                }
        } else {
            for (int c = 0; c < C; ++c) {
                float g;
                pixel_term<KIND>(to_f32(pa[c]) - to_f32(pb[c]), eps, gscale, s, g);
                if (pg) pg[c] = from_f32<T>(g);
            }
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0 && loss_out) emit(loss_out, (float)(s * (double)gscale), det);
}

// sgn = -1 where the term is of -x (target_is_real of wgan / wgan_softplus / the discriminator's hinge, and the generator's hinge), else +1
template <int FORM> __device__ __forceinline__ void gan_term(float v, float sgn, float target, float gscale, double& s, float& g) {
    if constexpr (FORM == GAN_LSGAN) {
        const float d = v - target;
        s += (double)(d * d);
        g = 2.f * gscale * d;
    } else if constexpr (FORM == GAN_LINEAR) {
        s += (double)(sgn * v);
        g = sgn * gscale;
    } else if constexpr (FORM == GAN_SOFTPLUS) {
        const float z = sgn * v;
        s += (double)(fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))));      // softplus(z), finite for every finite z
        g = sgn * gscale / (1.f + expf(-z));                            // sigmoid(z): exp overflows to +inf only where the quotient is 0
    } else {
        const float h = 1.f + sgn * v;
        s += (double)fmaxf(h, 0.f);
        g = h > 0.f ? sgn * gscale : 0.f;                               // relu'(0) = 0, as torch
    }
}

// gscale = weight / npix; one logit per pixel (the discriminator's output is channel 0 of an 8-channel NHWC buffer)
template <typename T, int FORM>
__global__ __launch_bounds__(NT) void gan_loss_kernel(ssr_view x, ssr_view grad, long npix, float sgn, float target, float gscale,
                                                      float invn, float* __restrict__ loss_out, float* __restrict__ mean_out, bool det) {
    __shared__ double sh[NT / 64];
    const T* __restrict__ xp = reinterpret_cast<const T*>(x.p) + x.coff;
    T* __restrict__ gp = grad.p ? reinterpret_cast<T*>(grad.p) + grad.coff : nullptr;
    double s = 0.0, sm = 0.0;
    for (long p = (long)blockIdx.x * NT + threadIdx.x; p < npix; p += (long)gridDim.x * NT) {
        const float f = to_f32(xp[p * x.cs]);
        float g;
        gan_term<FORM>(f, sgn, target, gscale, s, g);
        sm += (double)f;
        if (gp) gp[p * grad.cs] = from_f32<T>(g);
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0 && loss_out) emit(loss_out, (float)(s * (double)gscale), det);
    if (mean_out) {
        sm = block_sum(sm, sh);
        if (threadIdx.x == 0) emit(mean_out, (float)(sm * (double)invn), det);
    }
}

inline int grid_of(long items, bool det) {
    long g = (items + SPAN - 1) / SPAN;
    const long cap = det ? SSR_LOSS_SLOTS : CAP;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// the four elements at coff .. coff + 3 of every pixel of the view are one aligned group inside the pixel's cs elements
inline bool group_of_four(const ssr_view& v, size_t elem) {
    return v.cs % 4 == 0 && v.coff % 4 == 0 && v.coff + 4 <= v.cs && ((uintptr_t)v.p % (4 * elem)) == 0;
}
}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

template <typename T, int KIND>
static void launch_pixel(bool vec, int g, void* stream, ssr_view a, ssr_view b, ssr_view grad, long npix, int C, float eps, float gscale,
                         float* loss_out, bool det) {
    if (vec)
        hipLaunchKernelGGL((pixel_loss_kernel<T, KIND, true>), dim3(g), dim3(NT), 0, ST(stream), a, b, grad, npix, C, eps, gscale, loss_out, det);
    else
        hipLaunchKernelGGL((pixel_loss_kernel<T, KIND, false>), dim3(g), dim3(NT), 0, ST(stream), a, b, grad, npix, C, eps, gscale, loss_out, det);
}

extern "C" int ssr_pixel_loss(ssr_view a, ssr_view b, ssr_view grad, int32_t dtype, int64_t npix, int32_t C, int32_t kind, float eps,
                              float weight, float* loss_out, void* stream) {
    const bool det = (dtype & SSR_DETERMINISTIC) != 0;      // loss_out = SSR_LOSS_SLOTS floats, one per block
    dtype &= ~SSR_DETERMINISTIC;
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!a.p || !b.p || npix <= 0 || C <= 0 || !(eps >= 0.f)) return SSR_EINVAL;
    if (a.coff < 0 || a.coff + C > a.cs || b.coff < 0 || b.coff + C > b.cs) return SSR_EINVAL;
    if (grad.p && (grad.coff < 0 || grad.coff + C > grad.cs)) return SSR_EINVAL;
    if (dtype != SSR_F32 && dtype != SSR_BF16) return SSR_EUNSUP;
    if (kind != PIX_MSE && kind != PIX_CHARBONNIER) return SSR_EUNSUP;
    const int g = grid_of((long)npix, det);
    const float gscale = (float)((double)weight / ((double)npix * C));
    const size_t elem = dtype == SSR_F32 ? 4 : 2;
    const bool vec = C <= 4 && group_of_four(a, elem) && group_of_four(b, elem);
    if (dtype == SSR_F32) {
        if (kind == PIX_MSE) launch_pixel<float, PIX_MSE>(vec, g, stream, a, b, grad, (long)npix, C, eps, gscale, loss_out, det);
        else launch_pixel<float, PIX_CHARBONNIER>(vec, g, stream, a, b, grad, (long)npix, C, eps, gscale, loss_out, det);
    } else {
        if (kind == PIX_MSE) launch_pixel<__bf16, PIX_MSE>(vec, g, stream, a, b, grad, (long)npix, C, eps, gscale, loss_out, det);
        else launch_pixel<__bf16, PIX_CHARBONNIER>(vec, g, stream, a, b, grad, (long)npix, C, eps, gscale, loss_out, det);
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

template <typename T>
static void launch_gan(int form, int g, void* stream, ssr_view x, ssr_view grad, long npix, float sgn, float target, float gscale,
                       float invn, float* loss_out, float* mean_out, bool det) {
#define SSR_GAN_FORM(F)                                                                                                             \
    hipLaunchKernelGGL((gan_loss_kernel<T, F>), dim3(g), dim3(NT), 0, ST(stream), x, grad, npix, sgn, target, gscale, invn, loss_out, \
                       mean_out, det)
    switch (form) {
    case GAN_LSGAN: SSR_GAN_FORM(GAN_LSGAN); break;
    case GAN_LINEAR: SSR_GAN_FORM(GAN_LINEAR); break;
    case GAN_SOFTPLUS: SSR_GAN_FORM(GAN_SOFTPLUS); break;
    default: SSR_GAN_FORM(GAN_HINGE_D); break;
    }
#undef SSR_GAN_FORM
}

extern "C" int ssr_gan_loss(ssr_view x, ssr_view grad, int32_t dtype, int64_t npix, int32_t gan_type, int32_t target_is_real,
                            int32_t is_disc, float target_val, float weight, float* loss_out, float* mean_out, void* stream) {
    const bool det = (dtype & SSR_DETERMINISTIC) != 0;      // loss_out / mean_out = SSR_LOSS_SLOTS floats each, one per block
    dtype &= ~SSR_DETERMINISTIC;
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!x.p || npix <= 0) return SSR_EINVAL;
    if (x.coff < 0 || x.coff + 1 > x.cs) return SSR_EINVAL;
    if (grad.p && (grad.coff < 0 || grad.coff + 1 > grad.cs)) return SSR_EINVAL;
    if (dtype != SSR_F32 && dtype != SSR_BF16) return SSR_EUNSUP;
    if (gan_type < 1 || gan_type > 4) return SSR_EUNSUP;
    // GANLoss.forward: the generator's hinge term is -input.mean() whatever target_is_real, i.e. wgan's real side
    const bool hinge_g = gan_type == 4 && !is_disc;
    const int form = gan_type == 1 ? GAN_LSGAN : (gan_type == 2 || hinge_g) ? GAN_LINEAR : gan_type == 3 ? GAN_SOFTPLUS : GAN_HINGE_D;
    const float sgn = (target_is_real || hinge_g) ? -1.f : 1.f;
    const int g = grid_of((long)npix, det);
    const float gscale = (float)((double)weight / (double)npix), invn = (float)(1.0 / (double)npix);
    if (dtype == SSR_F32) launch_gan<float>(form, g, stream, x, grad, (long)npix, sgn, target_val, gscale, invn, loss_out, mean_out, det);
    else launch_gan<__bf16>(form, g, stream, x, grad, (long)npix, sgn, target_val, gscale, invn, loss_out, mean_out, det);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
