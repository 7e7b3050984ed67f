// SSIM loss of train.ssim_opt (type SSIMLoss; reference: ssr/losses/basic_loss.py:50-60, called at ssr_esrgan_model.py:163-166):
// loss_weight * mean(clamp((1 - S) / 2, 0, 1)) with S the 5 x 5 Gaussian-window (sigma 1.5) SSIM over 2-pixel reflect padding,
// C1 = 1e-4, C2 = 9e-4, eps = 1e-12 - and its gradient with respect to x, in ONE launch (ssr_ssim_loss, include/ssr_hip.h; the CPU
// statement is satlas_super_resolution_amd/ssim_loss.py).
//
// One workgroup of 1024 threads per (image, 32 x 32 tile), every tile walked channel group by channel group (3 channels staged at
// a time, their positions worked on side by side: 3 x 36 x 36 moment items, 3 x 32 x 32 gradient items):
//   1. x and y of the tile + 4 pixels of halo -> LDS as fp32 (one thread reads the channels of one pixel: the strided NHWC lines are
//      fetched once per group, not once per channel)
//   2. on tile + 2: the five window moments with the reflected taps read straight from LDS, each taken about the window's own
//      centre pixel (sums of g (x - x0), g (x - x0)^2, ...): variances and the covariance come out without the
//      E[x^2] - E[x]^2 cancellation, exactly 0 in flat regions; from them S, the loss of the tile's own pixels, and the three
//      coefficient images a, b, c' = c + 2 b (0 outside the image and where the clamp is active) -> LDS.  B1 - A1 = (mx - my)^2 and
//      B2 - A2 = var(x - y) are formed directly, 1 - S from them: where x == y the loss is eps / D and the gradient 0, not rounding
//      noise of terms of size 1 / C2
//   3. d l / d x = Ft(a) + 2 x Ft(b) + y Ft(c) = Ft(a) + 2 (x - y) Ft(b) + y Ft(c') per tile pixel: Ft, the TRANSPOSE of the reflect-padded filter, reaches no further than
//      2 pixels either (the taps folded in from the padding land on rows 1, 2, n-3, n-2 from sources at most 2 away), so it is a
//      5 x 5 gather with per-row / per-column weights  w(p, q) = sum of g[t] over t with reflect(q + t) == p.  No float atomics:
//      every gradient element has one writer and a fixed order of additions.
// All arithmetic is fp32 whatever the storage type.
#include "common.h"

namespace {

constexpr int TS = 32;            // tile edge
constexpr int XW = TS + 8;        // staged x / y: tile + 4
constexpr int AW = TS + 4;        // moments and a, b, c: tile + 2
constexpr int CG = 3;             // channels staged per pass
constexpr int NT = 1024;          // threads of a workgroup: under SSR_DETERMINISTIC at most SSR_LOSS_SLOTS workgroups run, one per CU
constexpr size_t LDS_BYTES = (size_t)(2 * CG * XW * XW + CG * 3 * AW * AW + 2 * TS * 5) * sizeof(float);   // 86 336
constexpr float G0 = 0.29208171834287244f, G1 = 0.2338807565853503f, G2 = 0.12007838424321347f;   // exp(-t^2 / 4.5) / sum, |t| = 0, 1, 2
constexpr float SSIM_C1 = 1e-4f, SSIM_C2 = 9e-4f, SSIM_EPS = 1e-12f;

__device__ __forceinline__ float gauss(int t) { return t == 0 ? G0 : ((t == 1 || t == -1) ? G1 : G2); }   // |t| <= 2
__device__ __forceinline__ int reflect(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v); }

// weight of source q in Ft's output p along an axis of length n >= 3: every tap t in -2 .. 2 of F's row q that lands on p, directly
// (q + t == p) or folded from the padding (q + t == -p for p in 1 .. 2; q + t == 2 (n - 1) - p where that lies in n .. n + 1)
__device__ __forceinline__ float ft_weight(int p, int q, int n) {
    if (q < 0 || q >= n) return 0.f;
    float w = 0.f;
    int t = p - q;
    if (t >= -2 && t <= 2) w += gauss(t);
    if (p >= 1 && p <= 2) {
        t = -p - q;                       // <= -1
        if (t >= -2) w += gauss(t);
    }
    if (p <= n - 2 && p >= n - 3) {
        t = 2 * (n - 1) - p - q;          // >= 1
        if (t <= 2) w += gauss(t);
    }
    return w;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__global__ __launch_bounds__(NT) void ssim_loss_kernel(ssr_view x, ssr_view y, ssr_view grad, int N, int H, int W, int C, int tiles_y,
                                                       int tiles_x, float loss_scale, float grad_scale, int accumulate,
                                                       float* __restrict__ loss_out, bool det) {
    extern __shared__ __align__(16) float lds[];
    float* __restrict__ xs = lds;                         // [CG][XW * XW]
    float* __restrict__ ys = xs + CG * XW * XW;           // [CG][XW * XW]
    float* __restrict__ abc = ys + CG * XW * XW;          // [CG][3][AW * AW]: a, b, c' = c + 2 b
    float* __restrict__ wrow = abc + CG * 3 * AW * AW;    // [TS][5]: Ft's weights of the tile's rows ...
    float* __restrict__ wcol = wrow + TS * 5;             // [TS][5]: ... and columns
    __shared__ float sh[NT / 64];
    const T* __restrict__ xp = reinterpret_cast<const T*>(x.p);
    const T* __restrict__ yp = reinterpret_cast<const T*>(y.p);
    T* __restrict__ gp = reinterpret_cast<T*>(grad.p);
    const int tid = threadIdx.x;
    const long ntiles = (long)N * tiles_y * tiles_x;
    float lsum = 0.f;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int tx = (int)(tile % tiles_x), ty = (int)((tile / tiles_x) % tiles_y), n = (int)(tile / ((long)tiles_x * tiles_y));
        const int y0 = ty * TS, x0 = tx * TS;
        for (int c0 = 0; c0 < C; c0 += CG) {
            const int cg = min(CG, C - c0);
            __syncthreads();                  // the previous pass has read xs / ys / abc / the weights
            for (int i = tid; i < XW * XW; i += NT) {
                const int r = i / XW, cc = i - r * XW;
                const int gy = y0 - 4 + r, gx = x0 - 4 + cc;
                const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
                const long pix = ((long)n * H + gy) * W + gx;
#pragma unroll
                for (int j = 0; j < CG; ++j) {
                    const bool ld = in && j < cg;                 // channels >= C and pixels outside the image are never read
                    xs[j * XW * XW + i] = ld ? to_f32(xp[pix * x.cs + x.coff + c0 + j]) : 0.f;
                    ys[j * XW * XW + i] = ld ? to_f32(yp[pix * y.cs + y.coff + c0 + j]) : 0.f;
                }
            }
            if (tid < 2 * TS * 5) {           // Ft's weights: entry (p, t) of a row / column p of the tile is the weight of source p + t - 2
                const int k = tid < TS * 5 ? tid : tid - TS * 5, p = k / 5, t = k - p * 5;
                if (tid < TS * 5) wrow[k] = ft_weight(y0 + p, y0 + p + t - 2, H);
                else wcol[k] = ft_weight(x0 + p, x0 + p + t - 2, W);
            }
            __syncthreads();
            // every (channel, position) of tile + 2 is one work item
            for (int it = tid; it < cg * AW * AW; it += NT) {
                const int j = it / (AW * AW), i = it - j * AW * AW;
                const float* __restrict__ xj = xs + j * XW * XW;
                const float* __restrict__ yj = ys + j * XW * XW;
                const int r = i / AW, cc = i - r * AW;
                const int gy = y0 - 2 + r, gx = x0 - 2 + cc;
                float av = 0.f, bv = 0.f, cv = 0.f;
                if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                    int ro[5], co[5];     // LDS row offsets / columns of the five reflected taps (all within 2 of the centre)
#pragma unroll
                    for (int t = 0; t < 5; ++t) {
                        ro[t] = (reflect(gy + t - 2, H) - (y0 - 4)) * XW;
                        co[t] = reflect(gx + t - 2, W) - (x0 - 4);
                    }
                    const float xc = xj[(r + 2) * XW + cc + 2], yc = yj[(r + 2) * XW + cc + 2];
                    float sx = 0.f, sy = 0.f, sxy = 0.f, sdd = 0.f;
#pragma unroll
                    for (int u = 0; u < 5; ++u) {
                        float rx = 0.f, ry = 0.f, rxy = 0.f, rdd = 0.f;
#pragma unroll
                        for (int v = 0; v < 5; ++v) {
                            const float g = gauss(v - 2);
                            const float dx = xj[ro[u] + co[v]] - xc, dy = yj[ro[u] + co[v]] - yc;
                            const float dd = dx - dy;
                            rx += g * dx; ry += g * dy;
                            rxy += g * dx * dy; rdd += g * dd * dd;
                        }
                        const float g = gauss(u - 2);
                        sx += g * rx; sy += g * ry; sxy += g * rxy; sdd += g * rdd;
                    }
                    const float mx = xc + sx, my = yc + sy;
                    // B1 = A1 + d1 and B2 = A2 + d2 with d1 = (mx - my)^2, d2 = var(x - y): both exactly 0 where x == y
                    const float dm = mx - my, ds = sx - sy;
                    const float d1 = dm * dm, d2 = sdd - ds * ds;
                    const float A1 = 2.f * mx * my + SSIM_C1;
                    const float A2 = 2.f * (sxy - sx * sy) + SSIM_C2;
                    const float B1 = A1 + d1, B2 = A2 + d2;
                    const float D = B1 * B2 + SSIM_EPS;
                    const float invD = 1.f / D;
                    // (1 - S) / 2 = (D - A1 A2) / (2 D), a sum of non-negative terms (never below the clamp's lower side)
                    const float l = 0.5f * (A1 * d2 + B2 * d1 + SSIM_EPS) * invD;
                    const float S = 1.f - 2.f * l;
                    if (l <= 1.f) {                   // torch's clamp gradient: 1 on the closed interval, 0 outside
                        // a = (2 my (A2 - A1) - 2 mx S (B2 - B1)) / D regrouped around the differences above, and c' = c + 2 b
                        // = 2 (A1 - S B1) / D, so that the large terms that cancel where x ~ y are never formed:
                        // d l / d x = Ft(a) + 2 (x - y) Ft(b) + y Ft(c')
                        av = 2.f * (-dm * (A2 - A1) - mx * (d2 - d1) + 2.f * mx * l * (B2 - B1)) * invD;
                        bv = -S * B1 * invD;
                        cv = 2.f * (2.f * l * B1 - d1) * invD;
                    }
                    if (r >= 2 && r < TS + 2 && cc >= 2 && cc < TS + 2) lsum += fminf(fmaxf(l, 0.f), 1.f);   // the tile's own pixels
                }
                float* __restrict__ o = abc + j * 3 * AW * AW + i;
                o[0] = av; o[AW * AW] = bv; o[2 * AW * AW] = cv;
            }
            __syncthreads();
            // every (channel, pixel) of the tile is one work item
            if (gp) for (int it = tid; it < cg * TS * TS; it += NT) {
                const int j = it / (TS * TS), p = it - j * TS * TS;
                const int r = p / TS, cc = p - r * TS;
                const int gy = y0 + r, gx = x0 + cc;
                if (gy >= H || gx >= W) continue;
                const float* __restrict__ aj = abc + j * 3 * AW * AW;
                float wx[5];
#pragma unroll
                for (int v = 0; v < 5; ++v) wx[v] = wcol[cc * 5 + v];
                float fa = 0.f, fb = 0.f, fc = 0.f;
#pragma unroll
                for (int u = 0; u < 5; ++u) {
                    const float wy = wrow[r * 5 + u];
                    float ra = 0.f, rb = 0.f, rc = 0.f;
#pragma unroll
                    for (int v = 0; v < 5; ++v) {
                        const int q = (r + u) * AW + cc + v;
                        ra += wx[v] * aj[q]; rb += wx[v] * aj[AW * AW + q]; rc += wx[v] * aj[2 * AW * AW + q];
                    }
                    fa += wy * ra; fb += wy * rb; fc += wy * rc;
                }
                const int ci = j * XW * XW + (r + 4) * XW + cc + 4;
                const float g = grad_scale * (fa + 2.f * (xs[ci] - ys[ci]) * fb + ys[ci] * fc);
                const long o = (((long)n * H + gy) * W + gx) * grad.cs + grad.coff + c0 + j;
                gp[o] = from_f32<T>(accumulate ? to_f32(gp[o]) + g : g);     // bf16: the sum is rounded once
            }
        }
    }
    // block sum in a fixed order; det: slot b has one writer per launch (the reader adds the slots in index order), default: one
    // fp32 atomic per block, as ssr_l1_loss
    lsum = wave_sum(lsum);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = lsum;
    __syncthreads();
    if (tid == 0 && loss_out) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) s += sh[k];
        s *= loss_scale;
        if (det) loss_out[blockIdx.x] += s; else atomicAdd(loss_out, s);
    }
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_ssim_loss(ssr_view x, ssr_view y, ssr_view grad, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C,
                             float weight, int32_t accumulate, float* loss_out, void* stream) {
    const bool det = (dtype & SSR_DETERMINISTIC) != 0;      // loss_out = SSR_LOSS_SLOTS floats, one per block
    dtype &= ~SSR_DETERMINISTIC;
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!x.p || !y.p || N <= 0 || C <= 0 || H < 3 || W < 3) return SSR_EINVAL;     // 2-pixel reflect padding needs 3 pixels
    if (x.coff < 0 || x.coff + C > x.cs || y.coff < 0 || y.coff + C > y.cs) return SSR_EINVAL;
    if (grad.p && (grad.coff < 0 || grad.coff + C > grad.cs)) return SSR_EINVAL;
    if (dtype != SSR_F32 && dtype != SSR_BF16) return SSR_EUNSUP;
    const int tiles_y = (H + TS - 1) / TS, tiles_x = (W + TS - 1) / TS;
    const long ntiles = (long)N * tiles_y * tiles_x;
    const long cap = det ? SSR_LOSS_SLOTS : 65536;
    const int g = (int)(ntiles < cap ? ntiles : cap);
    static bool attr_done[SSR_MAX_DEVICES] = {};      // the attribute is per DEVICE
    const int attr_dev = ssr_device_ordinal();
    if (!attr_done[attr_dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_loss_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_loss_kernel<__bf16>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        attr_done[attr_dev] = true;
    }
    const double total = (double)N * H * W * C;
    const float loss_scale = (float)((double)weight / total), grad_scale = (float)(-(double)weight / (2.0 * total));
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(ssim_loss_kernel<float>, dim3(g), dim3(NT), LDS_BYTES, ST(stream), x, y, grad, N, H, W, C, tiles_y, tiles_x,
                           loss_scale, grad_scale, accumulate, loss_out, det);
    else
        hipLaunchKernelGGL(ssim_loss_kernel<__bf16>, dim3(g), dim3(NT), LDS_BYTES, ST(stream), x, y, grad, N, H, W, C, tiles_y, tiles_x,
                           loss_scale, grad_scale, accumulate, loss_out, det);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
