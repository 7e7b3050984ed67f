// The tower linears on split operands: ssr_linear's product with the contraction on the 16-bit matrix core (include/ssr_hip.h).
//
//   ssr_linear_split_pack   W [Nout][K] fp32 -> hi and lo 16-bit pieces, once, at load
//   ssr_linear_split        Y = act(X W^T + b) (+ R): per 16 k, x_hi w_hi + x_hi w_lo + x_lo w_hi on v_mfma_f32_32x32x16_f16 / _bf16
//
// Packed weight layout (`wpk`), KG = ceil(K / 8) groups of 8 consecutive k per row of W:
//     wpk[n][kg] = 32 bytes: [ 8 hi pieces of W[n][8 kg .. 8 kg + 7] | the 8 lo pieces ],   n < Nout, kg < KG, row-major
// k >= K inside the last group is stored as zeros.  SSR_SPLIT_F16: the pieces are fp16 and W is multiplied by SSR_F32H_WSCALE (2^10)
// before the split; SSR_SPLIT_BF16: bf16 pieces, no scale.  One 16-byte half of an entry is exactly what one lane feeds the MFMA as
// its B operand (lane l: B[k = 8 (l >> 5) + j][col l & 31]), so the kernel moves entries into LDS and from LDS into registers as they are.
//
// Determinism: no atomics, no split-K.  Per output ONE fp32 accumulator, k groups of 16 ascending, within a group hi hi, hi lo, lo hi.
// The tile shape is chosen from M and Nout, but every output is the same chain over the same operands whatever the tile or its place.
#include "common.h"
#include "vit_act.h"

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool view_ok(const ssr_view& v, int c) {
    return v.p && v.coff >= 0 && v.cs >= v.coff + c && !(v.cs % 4) && !(v.coff % 4) && aligned16(v.p);
}

// ---------------------------------------------------------------------------------------------- pack
// one thread per (n, kg): two float4 reads (the second masked by K), two 16-byte stores
template <bool H> __global__ __launch_bounds__(256) void linear_split_pack_kernel(const float* __restrict__ w, int Nout, int K, int KG,
                                                                                  u32x4* __restrict__ out) {
    const long total = (long)Nout * KG;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i / KG), kg = (int)(i - (long)n * KG);
        u32x4 hi, lo;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 8 * kg + 4 * h;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < K) v = *reinterpret_cast<const f32x4*>(w + (long)n * K + k);
            if constexpr (H) v *= SSR_F32H_WSCALE;
            uint2 ph, pl;
            split_f32x4<H>(__builtin_bit_cast(u32x4, v), ph, pl);
            hi[2 * h] = ph.x, hi[2 * h + 1] = ph.y;
            lo[2 * h] = pl.x, lo[2 * h + 1] = pl.y;
        }
        out[2 * i] = hi;
        out[2 * i + 1] = lo;
    }
}

// ---------------------------------------------------------------------------------------------- ssr_linear_split
// Block: 256 threads = 2 x 2 waves, each wave TM x TN MFMA tiles of 32 x 32 -> a (64 TM) x (64 TN) tile of Y; K in steps of 32 = 4 groups
// of 8.  A operand X (lane (i, g): X[m = i][k = 8 g + j]), B operand W (W[n = i][k = 8 g + j]): a lane ends with column n = lane & 31 and
// rows mfma32_row(e, g), as ssr_linear.
// LDS: four arrays of 16-byte chunks (X hi, X lo, W hi, W lo), chunk [kg][row] = the 8 pieces of that row and k group.  An operand read
// is one ds_read_b128 per lane at [2 s + g][row]: the 16 lanes of a read group hold 16 rows that differ mod 16, i.e. 64 distinct banks.
// Staging: X is split here, a float4 (4 k) per item gives 8 bytes of hi and 8 of lo; items are dealt so that 16 consecutive lanes hold
// 8 rows x 2 halves of ONE k group (32 distinct banks per 8-byte store group).  W entries are copied: 8 consecutive lanes hold 8 rows of
// one k group (128 contiguous bytes per 16-byte store group).
// Tails: rows >= M, rows of W >= Nout and k >= K are staged as zeros (never read from memory) and never stored.
template <bool H, int TM, int TN>
__global__ __launch_bounds__(256) void linear_split_kernel(ssr_view x, const u32x4* __restrict__ wpk, const float* __restrict__ bias, ssr_view r,
                                                           ssr_view y, int M, int K, int Nout, int act) {
    constexpr int BM = 64 * TM, BN = 64 * TN, BK = 32, NKG = 4, XI = 2 * TM, WI = TN;
    __shared__ u32x4 sXh[NKG * BM], sXl[NKG * BM], sWh[NKG * BN], sWl[NKG * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, li = lane & 31, lg = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN, KG = (K + 7) >> 3;
    const float* __restrict__ xp = reinterpret_cast<const float*>(x.p) + x.coff;
    const u32x4 zero = {0u, 0u, 0u, 0u};
    u32x4 px[XI], pwh[WI], pwl[WI];

    // item f of X: half h = f & 1, row = 8 (f >> 6) + ((f >> 1) & 7), k group (f >> 4) & 3;  item f of W: row = 8 (f >> 5) + (f & 7), k group (f >> 3) & 3
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int f = tid + 256 * i, row = 8 * (f >> 6) + ((f >> 1) & 7), k = k0 + 8 * ((f >> 4) & 3) + 4 * (f & 1), m = m0 + row;
            px[i] = (m < M && k < K) ? *reinterpret_cast<const u32x4*>(xp + (long)m * x.cs + k) : zero;
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const int f = tid + 256 * i, row = 8 * (f >> 5) + (f & 7), kg = (k0 >> 3) + ((f >> 3) & 3), n = n0 + row;
            const bool in = n < Nout && kg < KG;
            const u32x4* e = wpk + 2 * ((long)n * KG + kg);
            pwh[i] = in ? e[0] : zero;
            pwl[i] = in ? e[1] : zero;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    uint2* sXh2 = reinterpret_cast<uint2*>(sXh);
    uint2* sXl2 = reinterpret_cast<uint2*>(sXl);
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();                       // the previous step's operand reads are done
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const int f = tid + 256 * i, row = 8 * (f >> 6) + ((f >> 1) & 7), kg = (f >> 4) & 3, h = f & 1;
            uint2 hi, lo;
            split_f32x4<H>(px[i], hi, lo);
            sXh2[2 * (kg * BM + row) + h] = hi;
            sXl2[2 * (kg * BM + row) + h] = lo;
        }
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const int f = tid + 256 * i, row = 8 * (f >> 5) + (f & 7), kg = (f >> 3) & 3;
            sWh[kg * BN + row] = pwh[i];
            sWl[kg * BN + row] = pwl[i];
        }
        __syncthreads();
        if (k0 + BK < K) fetch(k0 + BK);       // the next step's global loads fly under this step's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (k0 + 16 * s >= K) break;       // uniform: a 16-group wholly past K holds zeros in both operands
            const int kg = 2 * s + lg;
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) {
                ah[a] = __builtin_bit_cast(bf16x8, sXh[kg * BM + (wm * TM + a) * 32 + li]);
                al[a] = __builtin_bit_cast(bf16x8, sXl[kg * BM + (wm * TM + a) * 32 + li]);
            }
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                bh[b] = __builtin_bit_cast(bf16x8, sWh[kg * BN + (wn * TN + b) * 32 + li]);
                bl[b] = __builtin_bit_cast(bf16x8, sWl[kg * BN + (wn * TN + b) * 32 + li]);
            }
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    acc[a][b] = split_mfma<H>(ah[a], bh[b], acc[a][b]);
                    acc[a][b] = split_mfma<H>(ah[a], bl[b], acc[a][b]);
                    acc[a][b] = split_mfma<H>(al[a], bh[b], acc[a][b]);
                }
        }
    }

    // the weight scale comes off, then the bias, then the activation, then the residual last
    float* yp = reinterpret_cast<float*>(y.p) + y.coff;                                    // no __restrict__: r may alias y
    const float* rp = r.p ? reinterpret_cast<const float*>(r.p) + r.coff : nullptr;      // may alias y (same element, read before the write)
#pragma unroll
    for (int b = 0; b < TN; ++b) {
        const int n = n0 + (wn * TN + b) * 32 + li;
        if (n >= Nout) continue;
        const float bn = bias ? bias[n] : 0.f;
#pragma unroll
        for (int a = 0; a < TM; ++a) {
            const int mb = m0 + (wm * TM + a) * 32;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = mb + mfma32_row(e, lg);
                if (m >= M) continue;
                float v = acc[a][b][e];
                if constexpr (H) v *= SSR_F32H_UNSCALE;
                if (bias) v += bn;
                v = vit_act(v, act);
                if (rp) v += rp[(long)m * r.cs + n];
                yp[(long)m * y.cs + n] = v;
            }
        }
    }
}

template <bool H>
void launch_linear_split(ssr_view x, const void* wpk, const float* bias, ssr_view r, ssr_view y, int M, int K, int Nout, int act, hipStream_t st) {
    const u32x4* w = reinterpret_cast<const u32x4*>(wpk);
    const long big = (long)((M + 127) / 128) * ((Nout + 127) / 128);
    if (big >= 256)        // enough 128 x 128 tiles for every compute unit; below that the 64 x 64 tile spreads the work wider
        hipLaunchKernelGGL((linear_split_kernel<H, 2, 2>), dim3((Nout + 127) / 128, (M + 127) / 128), dim3(256), 0, st, x, w, bias, r, y, M, K, Nout, act);
    else
        hipLaunchKernelGGL((linear_split_kernel<H, 1, 1>), dim3((Nout + 63) / 64, (M + 63) / 64), dim3(256), 0, st, x, w, bias, r, y, M, K, Nout, act);
}

}  // namespace

extern "C" int64_t ssr_linear_split_pack_bytes(int32_t Nout, int32_t K) {
    if (Nout <= 0 || K <= 0) return SSR_EINVAL;
    return (int64_t)Nout * ((K + 7) / 8) * 32;
}

extern "C" int ssr_linear_split_pack(const float* w, int32_t Nout, int32_t K, int32_t pieces, void* out, void* stream) {
    if (!w || !out || Nout <= 0 || K <= 0) return SSR_EINVAL;
    if (pieces != SSR_SPLIT_F16 && pieces != SSR_SPLIT_BF16) return SSR_EINVAL;
    if ((K % 4) || (Nout % 4) || Nout > (1 << 22)) return SSR_EUNSUP;
    if (!aligned16(w) || !aligned16(out)) return SSR_EINVAL;
    const int KG = (K + 7) / 8;
    const long blocks = ((long)Nout * KG + 255) / 256;
    const dim3 grid((unsigned)(blocks > 16384 ? 16384 : blocks));
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (pieces == SSR_SPLIT_F16)
        hipLaunchKernelGGL(linear_split_pack_kernel<true>, grid, dim3(256), 0, st, w, Nout, K, KG, reinterpret_cast<u32x4*>(out));
    else
        hipLaunchKernelGGL(linear_split_pack_kernel<false>, grid, dim3(256), 0, st, w, Nout, K, KG, reinterpret_cast<u32x4*>(out));
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_linear_split(ssr_view x, const void* wpk, const float* bias, ssr_view r, ssr_view y, int32_t pieces, int32_t M, int32_t K,
                                int32_t Nout, int32_t act, void* stream) {
    if (M <= 0 || K <= 0 || Nout <= 0 || !wpk) return SSR_EINVAL;
    if (act < SSR_VIT_ACT_NONE || act > SSR_VIT_ACT_GELU_ERF) return SSR_EINVAL;
    if (pieces != SSR_SPLIT_F16 && pieces != SSR_SPLIT_BF16) return SSR_EINVAL;
    if ((K % 4) || (Nout % 4)) return SSR_EUNSUP;
    if (!view_ok(x, K) || !view_ok(y, Nout) || !aligned16(wpk) || (bias && (reinterpret_cast<uintptr_t>(bias) & 3))) return SSR_EINVAL;
    if (r.p && !view_ok(r, Nout)) return SSR_EINVAL;
    if (M > (1 << 22) || Nout > (1 << 22)) return SSR_EUNSUP;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (pieces == SSR_SPLIT_F16) launch_linear_split<true>(x, wpk, bias, r, y, M, K, Nout, act, st);
    else launch_linear_split<false>(x, wpk, bias, r, y, M, K, Nout, act, st);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
