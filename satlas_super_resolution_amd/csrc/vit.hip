// The vision tower of the CLIPScore validation metric (`calculate_clipscore`: SigLIP ViT-SO400M-14 at 384 x 384, OpenAI CLIP ViT-B/16
// at 224 x 224; clipscore_metric.py holds the definition).  A ViT forward is a chain of row-matrix operations over [tokens, channels]
// buffers, so every entry here takes fp32 ROW views (ssr_view: pointer, row stride cs, channel offset coff): q, k and v are the three
// slices of one packed buffer, the class-token rows of a batch are a view with cs = T * C, and so on.
//
//   ssr_linear            Y = act(X W^T + b) (+ R)   v_mfma_f32_32x32x2_f32, one accumulator chain per output over k ascending
//   ssr_layernorm_fwd     rows of C, mean and variance in fp64 (two passes over registers), one wave per row
//   ssr_mha_fwd           softmax(q k^T scale) v per (image, head), tiled over the keys (running max / sum), plain fp32 FMA
//   ssr_vit_patch_input   uint8 image -> patch matrix: table-driven nearest resize, channel permutation, / 255, (x - mean) / std
//   ssr_vit_tokens        [class token |] patch rows, + position embedding
//   ssr_cosine_pairs      cosine similarity of feature pairs, fp64 sums in index order
//
// No float atomics and no split reductions anywhere: two launches give the same bytes, and what an image receives depends neither
// on the batch size nor on its place in the batch (ssr_linear's tile shape is chosen from M, but every output is the same chain
// of MFMA steps over the same operands whatever the tile).
#include "common.h"
#include "vit_act.h"
#include <math.h>

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// an fp32 row view of at least `c` channels, 16-byte aligned rows
inline bool view_ok(const ssr_view& v, int c) {
    return v.p && v.coff >= 0 && v.cs >= v.coff + c && !(v.cs % 4) && !(v.coff % 4) && aligned16(v.p);
}

// ---------------------------------------------------------------------------------------------- ssr_linear
// vit_act: vit_act.h (shared with the activation pass of vit_bwd.hip)
// Block: 256 threads = 2 x 2 waves, each wave TM x TN MFMA tiles of 32 x 32 -> a (64 TM) x (64 TN) tile of Y; K in steps of 16.
// The MFMA's A operand is X (lane (i, g) supplies X[m = i][k = g]), its B operand W (W[n = i][k = g]), so a lane ends with column
// n = lane & 31 and rows m = mfma32_row(r, g): the 32 lanes of a half wave store 128 contiguous bytes of one row of Y.
// LDS holds both tiles TRANSPOSED ([k][row], row stride 64 T + 4 words): an operand read is one ds_read_b32 per lane, 32 consecutive
// words per k (conflict-free), and the k-pairs of successive MFMAs are (0, 1), (2, 3), ...: k ascending.  The staging store of a
// global float4 (4 k of one row) puts its words 64 T + 4 apart: lanes (row & 15, k quarter) land in 64 different banks.
// Tails: rows >= M, rows of W >= Nout and k >= K are staged as zeros (never read from memory) and never stored.
template <int TM, int TN>
__global__ __launch_bounds__(256) void linear_kernel(ssr_view x, const float* __restrict__ w, const float* __restrict__ bias, ssr_view r,
                                                     ssr_view y, int M, int K, int Nout, int act) {
    constexpr int BM = 64 * TM, BN = 64 * TN, BK = 16, LDA = BM + 4, LDB = BN + 4;
    __shared__ float sX[BK * LDA];
    __shared__ float sW[BK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1, li = lane & 31, lg = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const float* __restrict__ xp = reinterpret_cast<const float*>(x.p) + x.coff;
    f32x4 px[TM], pw[TN];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int f = tid + 256 * i, row = f >> 2, k = k0 + 4 * (f & 3), m = m0 + row;
            px[i] = (m < M && k < K) ? *reinterpret_cast<const f32x4*>(xp + (long)m * x.cs + k) : zero;
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int f = tid + 256 * i, row = f >> 2, k = k0 + 4 * (f & 3), n = n0 + row;
            pw[i] = (n < Nout && k < K) ? *reinterpret_cast<const f32x4*>(w + (long)n * K + k) : zero;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

    fetch(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();                       // the previous step's operand reads are done
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int f = tid + 256 * i, row = f >> 2, kq = 4 * (f & 3);
#pragma unroll
            for (int j = 0; j < 4; ++j) sX[(kq + j) * LDA + row] = px[i][j];
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int f = tid + 256 * i, row = f >> 2, kq = 4 * (f & 3);
#pragma unroll
            for (int j = 0; j < 4; ++j) sW[(kq + j) * LDB + row] = pw[i][j];
        }
        __syncthreads();
        if (k0 + BK < K) fetch(k0 + BK);       // the next step's global loads fly under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float av[TM], bv[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) av[a] = sX[(kk + lg) * LDA + (wm * TM + a) * 32 + li];
#pragma unroll
            for (int b = 0; b < TN; ++b) bv[b] = sW[(kk + lg) * LDB + (wn * TN + b) * 32 + li];
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
    }

    // bias, then the activation, then the residual last
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
                if (bias) v += bn;
                v = vit_act(v, act);
                if (rp) v += rp[(long)m * r.cs + n];
                yp[(long)m * y.cs + n] = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- ssr_layernorm_fwd
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // butterfly: every lane ends with the same bits
    return v;
}

// one wave per row (4 rows per block); lane l holds the float4 at channels 4 (l + 64 i), i < 8: C <= 2048
__global__ __launch_bounds__(256) void layernorm_kernel(ssr_view x, const float* __restrict__ gamma, const float* __restrict__ beta, ssr_view y,
                                                        int rows, int C, double eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, C4 = C >> 2;
    if (row >= rows) return;                                               // a whole wave leaves; no block-wide barrier below
    const float* xp = reinterpret_cast<const float*>(x.p) + (long)row * x.cs + x.coff;         // no __restrict__: y may alias x
    float* yp = reinterpret_cast<float*>(y.p) + (long)row * y.cs + y.coff;
    f32x4 v[8];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            v[i] = *reinterpret_cast<const f32x4*>(xp + 4 * c4);
            s += ((double)v[i][0] + (double)v[i][1]) + ((double)v[i][2] + (double)v[i][3]);
        }
    }
    const double mean = wave_sum(s) / (double)C;
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (lane + 64 * i < C4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)v[i][j] - mean;
                q += d * d;
            }
        }
    const double rstd = 1.0 / sqrt(wave_sum(q) / (double)C + eps);        // biased variance
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c4), b = *reinterpret_cast<const f32x4*>(beta + 4 * c4);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (float)(((double)v[i][j] - mean) * rstd * (double)g[j] + (double)b[j]);
            *reinterpret_cast<f32x4*>(yp + 4 * c4) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------- ssr_mha_fwd
// One block: 64 queries of one (image, head); the keys and values pass through LDS 64 at a time (K and V of one SO400M head are
// 420 KB), with the running maximum m, running sum l and the unnormalised output kept per query row ("online softmax").
//   phase 1   S = Q K^T * scale: thread (tq, tk) forms the 4 x 4 entries rows 4 tq + a, columns tk + 16 b (float4 reads along d)
//   phase 2   the 4 threads of a row share its 64 logits: tile maximum, p = exp(s - m_new) written back over S, l = l alpha + sum p
//   phase 3   O = O alpha + P V: thread (row, part) owns the D / 4 output channels part D / 4 ...
// Keys past Tk are staged as zeros and their logits set to -inf (p = 0); query rows past Tq are computed on zeros and not stored.
constexpr int MHA_TQ = 64, MHA_TK = 64, MHA_LS = MHA_TK + 1;
template <int D> constexpr int mha_lds_bytes() { return (3 * 64 * (D + 4) + MHA_TQ * MHA_LS) * (int)sizeof(float); }

template <int D>
__global__ __launch_bounds__(256) void mha_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int Tq, int Tk, float scale) {
    constexpr int LD = D + 4, DQ = D / 4, D4 = D / 4;
    extern __shared__ float mha_lds[];
    float* sQ = mha_lds;
    float* sK = sQ + MHA_TQ * LD;
    float* sV = sK + MHA_TK * LD;
    float* sS = sV + MHA_TK * LD;
    const int tid = threadIdx.x, n = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * MHA_TQ;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    for (int f = tid; f < MHA_TQ * D4; f += 256) {
        const int row = f / D4, c4 = f - row * D4, t = q0 + row;
        *reinterpret_cast<f32x4*>(sQ + row * LD + 4 * c4) =
            t < Tq ? *reinterpret_cast<const f32x4*>(qp + ((long)n * Tq + t) * q.cs + 4 * c4) : zero;
    }

    const int tq = tid >> 4, tk = tid & 15;            // phase 1
    const int row = tid >> 2, part = tid & 3;          // phases 2 and 3
    float m_run = -INFINITY, l_run = 0.f;
    float o[DQ];
#pragma unroll
    for (int c = 0; c < DQ; ++c) o[c] = 0.f;

    for (int kt0 = 0; kt0 < Tk; kt0 += MHA_TK) {
        __syncthreads();                               // phase 3 of the previous tile has read sV and sS
        for (int f = tid; f < MHA_TK * D4; f += 256) {
            const int kr = f / D4, c4 = f - kr * D4, t = kt0 + kr;
            const bool ok = t < Tk;
            *reinterpret_cast<f32x4*>(sK + kr * LD + 4 * c4) = ok ? *reinterpret_cast<const f32x4*>(kp + ((long)n * Tk + t) * k.cs + 4 * c4) : zero;
            *reinterpret_cast<f32x4*>(sV + kr * LD + 4 * c4) = ok ? *reinterpret_cast<const f32x4*>(vp + ((long)n * Tk + t) * v.cs + 4 * c4) : zero;
        }
        __syncthreads();
        {
            float acc[4][4];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
#pragma unroll 2
            for (int kk = 0; kk < D; kk += 4) {
                f32x4 qa[4], kb[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) qa[a] = *reinterpret_cast<const f32x4*>(sQ + (4 * tq + a) * LD + kk);
#pragma unroll
                for (int b = 0; b < 4; ++b) kb[b] = *reinterpret_cast<const f32x4*>(sK + (tk + 16 * b) * LD + kk);
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[a][b] = fmaf(qa[a][j], kb[b][j], acc[a][b]);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    sS[(4 * tq + a) * MHA_LS + tk + 16 * b] = (kt0 + tk + 16 * b < Tk) ? acc[a][b] * scale : -INFINITY;
        }
        __syncthreads();
        {
            float* srow = sS + row * MHA_LS + 16 * part;
            float mt = srow[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) mt = fmaxf(mt, srow[j]);
            mt = fmaxf(mt, __shfl_xor(mt, 1, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 2, 64));
            const float m_new = fmaxf(m_run, mt);       // finite: the tile holds at least one key
            const float alpha = expf(m_run - m_new);    // first tile: exp(-inf) = 0
            float ps = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float p = expf(srow[j] - m_new);
                srow[j] = p;
                ps += p;
            }
            ps += __shfl_xor(ps, 1, 64);
            ps += __shfl_xor(ps, 2, 64);
            l_run = l_run * alpha + ps;
            m_run = m_new;
#pragma unroll
            for (int c = 0; c < DQ; ++c) o[c] *= alpha;
        }
        __syncthreads();
        {
            const float* prow = sS + row * MHA_LS;
            const float* vcol = sV + part * DQ;
            for (int j = 0; j < MHA_TK; ++j) {
                const float p = prow[j];
#pragma unroll
                for (int c = 0; c < DQ; c += 2) {
                    const float2 vv = *reinterpret_cast<const float2*>(vcol + j * LD + c);
                    o[c] = fmaf(p, vv.x, o[c]);
                    o[c + 1] = fmaf(p, vv.y, o[c + 1]);
                }
            }
        }
    }
    const int t = q0 + row;
    if (t < Tq) {
        float* yp = reinterpret_cast<float*>(y.p) + ((long)n * Tq + t) * y.cs + y.coff + h * D + part * DQ;
        const float inv = 1.0f / l_run;
#pragma unroll
        for (int c = 0; c < DQ; c += 2) {
            float2 ov;
            ov.x = o[c] * inv;
            ov.y = o[c + 1] * inv;
            *reinterpret_cast<float2*>(yp + c) = ov;
        }
    }
}

template <int D>
int launch_mha(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int N, int Tq, int Tk, int heads, float scale, hipStream_t st) {
    auto kern = mha_kernel<D>;
    constexpr int lds = mha_lds_bytes<D>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_done[SSR_MAX_DEVICES] = {};      // the attribute is per DEVICE
    const int dev = ssr_device_ordinal();
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        attr_done[dev] = true;
    }
    hipLaunchKernelGGL(kern, dim3((Tq + MHA_TQ - 1) / MHA_TQ, heads, N), dim3(256), lds, st, q, k, v, y, Tq, Tk, scale);
    return 0;
}

// ---------------------------------------------------------------------------------------------- glue
struct patch_args { int perm[3]; float mean[3], std[3]; int normalize; };

// one thread per element of the patch matrix; a table entry outside the image writes 0 and reads nothing
__global__ __launch_bounds__(256) void patch_input_kernel(const uint8_t* __restrict__ u, int H, int W, const int32_t* __restrict__ rowidx,
                                                          const int32_t* __restrict__ colidx, int grid, int p, ssr_view y, long total,
                                                          patch_args a) {
// (v - mean) / std: two roundings, as the host states it; a fused form would round once
#pragma clang fp contract(off)
    const int pp = p * p, KP = 3 * pp, gg = grid * grid;
    float* __restrict__ yp = reinterpret_cast<float*>(y.p) + y.coff;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long rowp = e / KP;
        const int col = (int)(e - rowp * KP), n = (int)(rowp / gg), gi = (int)(rowp - (long)n * gg), gy = gi / grid, gx = gi - gy * grid;
        const int c = col / pp, rem = col - c * pp, py = rem / p, px = rem - py * p;
        const int sy = rowidx[gy * p + py], sx = colidx[gx * p + px];
        float val = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            val = (float)u[(((long)n * H + sy) * W + sx) * 3 + a.perm[c]] / 255.0f;          // IEEE division
            if (a.normalize) val = (val - a.mean[c]) / a.std[c];
        }
        yp[rowp * y.cs + col] = val;
    }
}

// x[n T + t] = (t < ncls ? cls : e[n G + t - ncls]) + pos[t], T = ncls + G; one thread per float4
__global__ __launch_bounds__(256) void tokens_kernel(ssr_view e, const float* __restrict__ cls, const float* __restrict__ pos, ssr_view x,
                                                     int N, int G, int C) {
    const int ncls = cls ? 1 : 0, T = G + ncls, C4 = C >> 2;
    const long total = (long)N * T * C4;
    const float* __restrict__ ep = reinterpret_cast<const float*>(e.p) + e.coff;
    float* __restrict__ xp = reinterpret_cast<float*>(x.p) + x.coff;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long rowx = i / C4;
        const int c = 4 * (int)(i - rowx * C4), n = (int)(rowx / T), t = (int)(rowx - (long)n * T);
        const f32x4 a = t < ncls ? *reinterpret_cast<const f32x4*>(cls + c)
                                 : *reinterpret_cast<const f32x4*>(ep + ((long)n * G + t - ncls) * e.cs + c);
        const f32x4 b = *reinterpret_cast<const f32x4*>(pos + (long)t * C + c);
        *reinterpret_cast<f32x4*>(xp + rowx * x.cs + c) = a + b;
    }
}

// one thread per pair: three fp64 sums in index order (the products of two floats are exact in fp64)
__global__ __launch_bounds__(64) void cosine_kernel(ssr_view f, int N, int E, double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* __restrict__ a = reinterpret_cast<const float*>(f.p) + (long)n * f.cs + f.coff;
    const float* __restrict__ b = reinterpret_cast<const float*>(f.p) + ((long)N + n) * f.cs + f.coff;
    double dot = 0.0, na = 0.0, nb = 0.0;
    for (int i = 0; i < E; ++i) {
        const double x = (double)a[i], z = (double)b[i];
        dot += x * z;
        na += x * x;
        nb += z * z;
    }
    out[n] = dot / fmax(sqrt(na) * sqrt(nb), 1e-8);
}

inline int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define VIT_F32(dtype)                           \
    do {                                         \
        if (dtype == SSR_F32X3) dtype = SSR_F32; \
        if (dtype == SSR_BF16) return SSR_EUNSUP;\
        if (dtype != SSR_F32) return SSR_EINVAL; \
    } while (0)

extern "C" int ssr_linear(ssr_view x, const float* w, const float* bias, ssr_view r, ssr_view y, int32_t dtype, int32_t M, int32_t K,
                          int32_t Nout, int32_t act, void* stream) {
    VIT_F32(dtype);
    if (M <= 0 || K <= 0 || Nout <= 0 || !w) return SSR_EINVAL;
    if (act < SSR_VIT_ACT_NONE || act > SSR_VIT_ACT_GELU_ERF) return SSR_EINVAL;
    if ((K % 4) || (Nout % 4)) return SSR_EUNSUP;
    if (!view_ok(x, K) || !view_ok(y, Nout) || !aligned16(w) || (bias && (reinterpret_cast<uintptr_t>(bias) & 3))) return SSR_EINVAL;
    if (r.p && !view_ok(r, Nout)) return SSR_EINVAL;
    if (M > (1 << 22) || Nout > (1 << 22)) return SSR_EUNSUP;
    const hipStream_t st = ST(stream);
    const long big = (long)((M + 127) / 128) * ((Nout + 127) / 128);
    if (big >= 256)        // enough 128 x 128 tiles for every compute unit; below that the 64 x 64 tile spreads the work wider
        hipLaunchKernelGGL((linear_kernel<2, 2>), dim3((Nout + 127) / 128, (M + 127) / 128), dim3(256), 0, st, x, w, bias, r, y, M, K, Nout, act);
    else
        hipLaunchKernelGGL((linear_kernel<1, 1>), dim3((Nout + 63) / 64, (M + 63) / 64), dim3(256), 0, st, x, w, bias, r, y, M, K, Nout, act);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_layernorm_fwd(ssr_view x, const float* gamma, const float* beta, ssr_view y, int32_t dtype, int32_t rows, int32_t C,
                                 double eps, void* stream) {
    VIT_F32(dtype);
    if (rows <= 0 || C <= 0 || !gamma || !beta || !(eps >= 0.0)) return SSR_EINVAL;
    if ((C % 4) || C > 2048) return SSR_EUNSUP;
    if (!view_ok(x, C) || !view_ok(y, C) || !aligned16(gamma) || !aligned16(beta)) return SSR_EINVAL;
    hipLaunchKernelGGL(layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, ST(stream), x, gamma, beta, y, rows, C, eps);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_mha_fwd(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int32_t dtype, int32_t N, int32_t Tq, int32_t Tk, int32_t heads,
                           int32_t d, float scale, void* stream) {
    VIT_F32(dtype);
    if (N <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || !(scale == scale)) return SSR_EINVAL;
    if ((d % 8) || d > 128 || N > 65535 || heads > 65535 || Tq > (1 << 20) || Tk > (1 << 20)) return SSR_EUNSUP;
    const int C = heads * d;
    if (!view_ok(q, C) || !view_ok(k, C) || !view_ok(v, C) || !view_ok(y, C)) return SSR_EINVAL;
    const hipStream_t st = ST(stream);
    int rc = 0;
#define MHA_CASE(D) case D: rc = launch_mha<D>(q, k, v, y, N, Tq, Tk, heads, scale, st); break;
    switch (d) {
        MHA_CASE(8) MHA_CASE(16) MHA_CASE(24) MHA_CASE(32) MHA_CASE(40) MHA_CASE(48) MHA_CASE(56) MHA_CASE(64)
        MHA_CASE(72) MHA_CASE(80) MHA_CASE(88) MHA_CASE(96) MHA_CASE(104) MHA_CASE(112) MHA_CASE(120) MHA_CASE(128)
        default: return SSR_EUNSUP;
    }
#undef MHA_CASE
    if (rc) return rc;
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_vit_patch_input(const uint8_t* u, int32_t N, int32_t H, int32_t W, const int32_t* rowidx, const int32_t* colidx,
                                   int32_t grid, int32_t p, ssr_view y, int32_t dtype, const int32_t* perm, const float* mean,
                                   const float* std, void* stream) {
    VIT_F32(dtype);
    if (!u || !rowidx || !colidx || !perm || N <= 0 || H <= 0 || W <= 0 || grid <= 0 || p <= 0) return SSR_EINVAL;
    if ((mean == nullptr) != (std == nullptr)) return SSR_EINVAL;
    if (p > 64 || grid > 1024) return SSR_EUNSUP;
    if (!view_ok(y, 3 * p * p)) return SSR_EINVAL;
    patch_args a;
    for (int c = 0; c < 3; ++c) {
        if (perm[c] < 0 || perm[c] > 2) return SSR_EINVAL;
        if (mean && !(std[c] != 0.f)) return SSR_EINVAL;
        a.perm[c] = perm[c];
        a.mean[c] = mean ? mean[c] : 0.f;
        a.std[c] = mean ? std[c] : 1.f;
    }
    a.normalize = mean ? 1 : 0;
    const long total = (long)N * grid * grid * 3 * p * p;
    hipLaunchKernelGGL(patch_input_kernel, dim3(grid_for(total)), dim3(256), 0, ST(stream), u, H, W, rowidx, colidx, grid, p, y, total, a);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_vit_tokens(ssr_view e, const float* cls, const float* pos, ssr_view x, int32_t dtype, int32_t N, int32_t G, int32_t C,
                              void* stream) {
    VIT_F32(dtype);
    if (!pos || N <= 0 || G <= 0 || C <= 0) return SSR_EINVAL;
    if (C % 4) return SSR_EUNSUP;
    if (!view_ok(e, C) || !view_ok(x, C) || !aligned16(pos) || (cls && !aligned16(cls))) return SSR_EINVAL;
    hipLaunchKernelGGL(tokens_kernel, dim3(grid_for((long)N * (G + 1) * (C / 4))), dim3(256), 0, ST(stream), e, cls, pos, x, N, G, C);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_cosine_pairs(ssr_view f, int32_t dtype, int32_t N, int32_t E, double* out, void* stream) {
    VIT_F32(dtype);
    if (!f.p || !out || N <= 0 || E <= 0 || f.coff < 0 || f.cs < f.coff + E || (reinterpret_cast<uintptr_t>(f.p) & 3) ||
        (reinterpret_cast<uintptr_t>(out) & 7))
        return SSR_EINVAL;
    hipLaunchKernelGGL(cosine_kernel, dim3((N + 63) / 64), dim3(64), 0, ST(stream), f, N, E, out);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
