// Gram-matrix style term of the VGG19 perceptual loss (BasicSR PerceptualLoss with style_weight > 0 and criterion 'l1', taken by
// ssr_esrgan_model.py:154-160 of the reference as l_g_style):
//
//   ssr_gram_fwd   G[n] = scale * F[n]^T F[n] over NHWC features F[n] = [H*W, C]: the contraction runs over the pixels.  Both MFMA
//                  operands are channel blocks of the same pixel chunk, staged channel-major in LDS (one tile feeds both on the
//                  diagonal); only the 64 x 64 tiles with i <= j are computed and every value is written to (i, j) and (j, i), so G is
//                  exactly symmetric.  Long contractions (conv1_2: 16384 pixels, 32 tiles at B = 32) are split over the pixels; each
//                  split writes a full partial matrix of its own and one pass adds the partials in split order (no float atomics:
//                  the same bytes from run to run in every mode).
//   ssr_gram_l1    loss += weight * sum |Gx - Gt| (per-block slots under SSR_DETERMINISTIC, as ssr_l1_loss); S = sign(Gx - Gt)
//                  (+1 / -1 / 0, exact in either storage type)
//   ssr_gram_bwd   gF[n] (+)= coef * F[n] S[n]: [H*W x C] x [C x C] per image; S is symmetric, so its rows serve as the columns
//
// Arithmetic: fp32 storage (SSR_F32 / SSR_F32X3) runs exact fp32 MFMA (v_mfma_f32_32x32x2_f32), bf16 storage bf16 MFMA
// (v_mfma_f32_32x32x16_bf16); both accumulate in fp32.  Each wave owns a 32 x 32 quarter of the workgroup's 64 x 64 tile.
#include "common.h"

namespace {

constexpr int GT = 64;     // output tile edge (channels, or pixels of the backward)
constexpr int KC = 32;     // contraction chunk staged in LDS per step
// LDS row = one tile row, KC contraction elements + pad: fp32 rows of 33 words (a 32-lane column read hits 32 banks),
// bf16 rows of 80 bytes (16-byte fragment reads stay aligned)
template <typename T> struct GramLd;
template <> struct GramLd<float> { static constexpr int LD = KC + 1; };
template <> struct GramLd<__bf16> { static constexpr int LD = KC + 8; };

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ float block_sum(float v, float* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < 64) {
        s = (threadIdx.x < nw) ? sh[threadIdx.x] : 0.f;
        s = wave_sum(s);
        if (threadIdx.x == 0) sh[0] = s;
    }
    __syncthreads();
    return sh[0];
}

// acc[i][j] += sum_k A[i][k] B[k][j] over one chunk, A[i][k] = As[i * LD + k], B[k][j] = Bs[j * LD + k] (both k-contiguous,
// 32 rows each from the given row 0)
template <typename T> __device__ __forceinline__ void mma_chunk(f32x16& acc, const T* As, const T* Bs);
template <> __device__ __forceinline__ void mma_chunk<float>(f32x16& acc, const float* As, const float* Bs) {
    constexpr int LD = GramLd<float>::LD;
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;      // lane: A[r][k = kb + h], B[k = kb + h][r]
#pragma unroll
    for (int kb = 0; kb < KC; kb += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[r * LD + kb + h], Bs[r * LD + kb + h], acc, 0, 0, 0);
}
template <> __device__ __forceinline__ void mma_chunk<__bf16>(f32x16& acc, const __bf16* As, const __bf16* Bs) {
    constexpr int LD = GramLd<__bf16>::LD;
    const int l = threadIdx.x & 63, r = l & 31, h = l >> 5;      // lane: A[r][k = kb + 8h + j], B[k = kb + 8h + j][r], j < 8
#pragma unroll
    for (int kb = 0; kb < KC; kb += 16) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(As + r * LD + kb + 8 * h);
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bs + r * LD + kb + 8 * h);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
}

// grid (upper tiles, splits, N); split s covers pixels [s * chunks_per * KC, +chunks_per * KC) and writes out + s * slab
template <typename T>
__global__ __launch_bounds__(256) void gram_fwd_kernel(ssr_view f, float* __restrict__ out, int P, int C, int chunks_per, float scale,
                                                       long slab) {
    constexpr int LD = GramLd<T>::LD, VEC = DT<T>::VEC, NV = KC * GT / VEC;
    typedef T vecT __attribute__((ext_vector_type(VEC)));
    __shared__ __align__(16) T xs[GT * LD];
    __shared__ __align__(16) T ys[GT * LD];
    const int CT = C / GT;
    int t = blockIdx.x, ti = 0;
    while (t >= CT - ti) { t -= CT - ti; ++ti; }
    const int tj = ti + t;
    const bool diag = ti == tj;
    const int s = blockIdx.y, n = blockIdx.z;
    const int pbeg = s * chunks_per * KC, pend = min(P, pbeg + chunks_per * KC);
    const int w = threadIdx.x >> 6, wi = w & 1, wj = w >> 1, l = threadIdx.x & 63;
    const bool idle = diag && wi > wj;           // the lower quarter of a diagonal tile is the mirror of the upper one
    const T* __restrict__ fp = reinterpret_cast<const T*>(f.p) + (long)n * P * f.cs + f.coff;
    const T* ysrc = diag ? xs : ys;
    f32x16 acc = {};
    for (int p0 = pbeg; p0 < pend; p0 += KC) {
        // F[p0 .. p0 + KC) x channels of block ti (and tj), transposed into LDS rows = channels; pixels past pend read as 0
        for (int v = threadIdx.x; v < (diag ? NV : 2 * NV); v += 256) {
            const int which = v >= NV, vv = which ? v - NV : v;
            const int p = vv / (GT / VEC), cv = vv % (GT / VEC);
            vecT x = {};
            if (p0 + p < pend) x = *reinterpret_cast<const vecT*>(fp + (long)(p0 + p) * f.cs + (which ? tj : ti) * GT + cv * VEC);
            T* dst = (which ? ys : xs) + cv * VEC * LD + p;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[e * LD] = x[e];
        }
        __syncthreads();
        if (!idle) mma_chunk<T>(acc, xs + wi * 32 * LD, ysrc + wj * 32 * LD);
        __syncthreads();
    }
    if (idle) return;
    float* __restrict__ o = out + s * slab + (long)n * C * C;
    const int j = tj * GT + wj * 32 + (l & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = ti * GT + wi * 32 + mfma32_row(r, l >> 5);
        if (i <= j) {
            const float v = acc[r] * scale;
            o[(long)i * C + j] = v;
            o[(long)j * C + i] = v;
        }
    }
}

// g[e] = scale * sum_{s < splits} ws[s * n + e], s in increasing order
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ ws, float* __restrict__ g, long n, int splits, float scale) {
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int p = 0; p < splits; ++p) s += ws[(long)p * n + e];
        g[e] = s * scale;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gram_l1_kernel(const float* __restrict__ gx, const float* __restrict__ gt, T* __restrict__ sgn, long n,
                                                      float weight, float* __restrict__ loss_out, bool det) {
    __shared__ float sh[16];
    float s = 0.f;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long)gridDim.x * blockDim.x) {
        const float d = gx[e] - gt[e];
        s += fabsf(d);
        if (sgn) sgn[e] = from_f32<T>(d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
    s = block_sum(s, sh);
    // det: slot b has one writer per launch (the reader adds the slots in index order); default: one fp32 atomic per block
    if (threadIdx.x == 0 && loss_out) { if (det) loss_out[blockIdx.x] += s * weight; else atomicAdd(loss_out, s * weight); }
}

// grid (pixel tiles, channel tiles, N): gF[n][p][c] (+)= coef * sum_d F[n][p][d] S[n][c][d]
template <typename T>
__global__ __launch_bounds__(256) void gram_bwd_kernel(ssr_view f, const T* __restrict__ sgn, ssr_view g, int P, int C, float coef,
                                                       int accumulate) {
    constexpr int LD = GramLd<T>::LD, VEC = DT<T>::VEC, NV = GT * KC / VEC;
    typedef T vecT __attribute__((ext_vector_type(VEC)));
    __shared__ __align__(16) T as[GT * LD];
    __shared__ __align__(16) T bs[GT * LD];
    const int p0 = blockIdx.x * GT, c0 = blockIdx.y * GT, n = blockIdx.z;
    const int w = threadIdx.x >> 6, wi = w & 1, wj = w >> 1, l = threadIdx.x & 63;
    const T* __restrict__ fp = reinterpret_cast<const T*>(f.p) + (long)n * P * f.cs + f.coff;
    const T* __restrict__ sp = sgn + (long)n * C * C;
    f32x16 acc = {};
    for (int d0 = 0; d0 < C; d0 += KC) {
        // rows: 64 pixels of F (past P read as 0) and 64 rows of S, each KC contraction channels wide
        for (int v = threadIdx.x; v < 2 * NV; v += 256) {
            const int which = v >= NV, vv = which ? v - NV : v;
            const int row = vv / (KC / VEC), kv = vv % (KC / VEC);
            vecT x = {};
            if (which) x = *reinterpret_cast<const vecT*>(sp + (long)(c0 + row) * C + d0 + kv * VEC);
            else if (p0 + row < P) x = *reinterpret_cast<const vecT*>(fp + (long)(p0 + row) * f.cs + d0 + kv * VEC);
            T* dst = (which ? bs : as) + row * LD + kv * VEC;
#pragma unroll
            for (int e = 0; e < VEC; ++e) dst[e] = x[e];
        }
        __syncthreads();
        mma_chunk<T>(acc, as + wi * 32 * LD, bs + wj * 32 * LD);
        __syncthreads();
    }
    T* __restrict__ gp = reinterpret_cast<T*>(g.p) + (long)n * P * g.cs + g.coff;
    const int c = c0 + wj * 32 + (l & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = p0 + wi * 32 + mfma32_row(r, l >> 5);
        if (p < P) {
            T* q = gp + (long)p * g.cs + c;
            float v = coef * acc[r];
            if (accumulate) v += to_f32(*q);
            *q = from_f32<T>(v);
        }
    }
}

inline int grid_for(long total, int per_block, int cap) {
    long g = (total + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// pixel splits of one Gram launch: enough workgroups for the chip (~1024) where the output has few tiles, at least 8 chunks
// (256 pixels) per split; returns the split count, chunks_per = chunks of each split (the last one may be shorter)
int gram_split(int N, int P, int C, int* chunks_per) {
    const int CT = C / GT, tiles = CT * (CT + 1) / 2, chunks = (P + KC - 1) / KC;
    const long base = (long)N * tiles;
    int s = (int)((1024 + base - 1) / base);
    s = max(1, min(s, chunks / 8));
    const int per = (chunks + s - 1) / s;
    if (chunks_per) *chunks_per = per;
    return (chunks + per - 1) / per;
}

bool gram_geom_ok(ssr_view f, int N, int P, int C, int vec) {
    return f.p && N > 0 && P > 0 && C > 0 && C % GT == 0 && f.cs >= f.coff + C && f.cs % vec == 0 && f.coff % vec == 0 && N <= 65535;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_gram_splits(int32_t N, int32_t HW, int32_t C) {
    if (N <= 0 || HW <= 0 || C <= 0 || C % GT) return SSR_EINVAL;
    return gram_split(N, HW, C, nullptr);
}

extern "C" int ssr_gram_fwd(ssr_view f, float* g, float* ws, int32_t dtype, int32_t N, int32_t HW, int32_t C, float scale, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32 && dtype != SSR_BF16) return SSR_EUNSUP;
    if (!g || !gram_geom_ok(f, N, HW, C, dtype == SSR_F32 ? 4 : 8)) return SSR_EINVAL;
    int per = 0;
    const int splits = gram_split(N, HW, C, &per);
    if (splits > 1 && !ws) return SSR_EINVAL;
    const int CT = C / GT;
    const long n = (long)N * C * C;
    float* out = splits > 1 ? ws : g;
    const float sc = splits > 1 ? 1.f : scale;
    const dim3 grid(CT * (CT + 1) / 2, splits, N);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(gram_fwd_kernel<float>, grid, dim3(256), 0, ST(stream), f, out, (int)HW, (int)C, per, sc, n);
    else
        hipLaunchKernelGGL(gram_fwd_kernel<__bf16>, grid, dim3(256), 0, ST(stream), f, out, (int)HW, (int)C, per, sc, n);
    SSR_LAUNCH_CHECK();
    if (splits > 1) {
        hipLaunchKernelGGL(gram_reduce_kernel, dim3(grid_for(n, 256 * 4, 2048)), dim3(256), 0, ST(stream), (const float*)ws, g, n, splits, scale);
        SSR_LAUNCH_CHECK();
    }
    return SSR_OK;
}

extern "C" int ssr_gram_l1(const float* gx, const float* gt, void* sgn, int32_t dtype, int64_t n, float weight, float* loss_out,
                           void* stream) {
    const bool det = (dtype & SSR_DETERMINISTIC) != 0;      // loss_out = SSR_LOSS_SLOTS floats, one per block
    dtype &= ~SSR_DETERMINISTIC;
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (!gx || !gt || n <= 0) return SSR_EINVAL;
    const int gr = grid_for(n, 256 * 4, det ? SSR_LOSS_SLOTS : 1024);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(gram_l1_kernel<float>, dim3(gr), dim3(256), 0, ST(stream), gx, gt, (float*)sgn, (long)n, weight, loss_out, det);
    else if (dtype == SSR_BF16)
        hipLaunchKernelGGL(gram_l1_kernel<__bf16>, dim3(gr), dim3(256), 0, ST(stream), gx, gt, (__bf16*)sgn, (long)n, weight, loss_out, det);
    else return SSR_EUNSUP;
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_gram_bwd(ssr_view f, const void* sgn, ssr_view gf, int32_t dtype, int32_t N, int32_t HW, int32_t C, float coef,
                            int32_t accumulate, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;
    if (dtype != SSR_F32 && dtype != SSR_BF16) return SSR_EUNSUP;
    const int vec = dtype == SSR_F32 ? 4 : 8;
    if (!sgn || !gram_geom_ok(f, N, HW, C, vec) || !gram_geom_ok(gf, N, HW, C, vec)) return SSR_EINVAL;
    const dim3 grid((HW + GT - 1) / GT, C / GT, N);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(gram_bwd_kernel<float>, grid, dim3(256), 0, ST(stream), f, (const float*)sgn, gf, (int)HW, (int)C, coef, (int)accumulate);
    else
        hipLaunchKernelGGL(gram_bwd_kernel<__bf16>, grid, dim3(256), 0, ST(stream), f, (const __bf16*)sgn, gf, (int)HW, (int)C, coef, (int)accumulate);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
