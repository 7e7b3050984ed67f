// The backward pass of the vision tower, for the CLIP loss of train.clip_opt (clip_loss.py holds the definition).  Only the gradient
// with respect to the IMAGE is formed: the tower's weights are not trained, so there is no weight-gradient kernel, and the linear
// data gradients dX = dY W are ssr_linear on weight copies transposed once at load.  Row views in exact fp32, as vit.hip.
//
//   ssr_vit_float_input       fp32 NHWC image -> patch matrix: table-driven nearest resize, channel permutation, (x - mean) / std
//   ssr_vit_float_input_bwd   its transpose in GATHER form: one thread per source element sums its destinations in index order
//   ssr_layernorm_bwd         dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma, statistics recomputed in fp64 (+ residual)
//   ssr_vit_act_fwd / _bwd    the activation as a pass of its own (vit_act.h) and dpre = dpost act'(pre)
//   ssr_mha_bwd               softmax attention backward: statistics recomputed over the key tiles, dq per query tile, dk / dv per key tile
//   ssr_feature_l1            weight * mean|fx - fg| (fp64, index order) and its gradient
//
// No float atomics and no split reductions: every output element has one writer and one fixed order of additions.
#include "common.h"
#include "vit_act.h"
#include <math.h>

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool view_ok(const ssr_view& v, int c) {
    return v.p && v.coff >= 0 && v.cs >= v.coff + c && !(v.cs % 4) && !(v.coff % 4) && aligned16(v.p);
}
inline int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

// ---------------------------------------------------------------------------------------------- the input pair
struct input_args { int perm[3]; float mean[3], std[3]; int normalize; };

// one thread per element of the patch matrix; a table entry outside the image writes 0 and reads nothing
__global__ __launch_bounds__(256) void float_input_kernel(ssr_view img, int H, int W, const int32_t* __restrict__ rowidx,
                                                          const int32_t* __restrict__ colidx, int grid, int p, ssr_view y, long total,
                                                          input_args a) {
// (v - mean) / std: two roundings, as ssr_vit_patch_input
#pragma clang fp contract(off)
    const int pp = p * p, KP = 3 * pp, gg = grid * grid;
    const float* __restrict__ ip = reinterpret_cast<const float*>(img.p) + img.coff;
    float* __restrict__ yp = reinterpret_cast<float*>(y.p) + y.coff;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long rowp = e / KP;
        const int col = (int)(e - rowp * KP), n = (int)(rowp / gg), gi = (int)(rowp - (long)n * gg), gy = gi / grid, gx = gi - gy * grid;
        const int c = col / pp, rem = col - c * pp, py = rem / p, px = rem - py * p;
        const int sy = rowidx[gy * p + py], sx = colidx[gx * p + px];
        float val = 0.f;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
            val = ip[(((long)n * H + sy) * W + sx) * img.cs + a.perm[c]];
            if (a.normalize) val = (val - a.mean[c]) / a.std[c];
        }
        yp[rowp * y.cs + col] = val;
    }
}

// One thread per SOURCE element (n, sy, sx, c): the destinations that read it are the rows rowrange[2 sy] .. rowrange[2 sy + 1] - 1 and
// the columns colrange[2 sx] .. colrange[2 sx + 1] - 1 of the resized image (half-open, clamped to the grid * p rows and columns the
// patch matrix holds; an empty range: the resize never reads this source).  fp64 sum, rows then columns ascending, one division by
// std, one fp32 rounding, then ONE fp32 addition into the gradient image (single writer: perm is a permutation).
__global__ __launch_bounds__(256) void float_input_bwd_kernel(ssr_view dpatch, int H, int W, const int32_t* __restrict__ rowrange,
                                                              const int32_t* __restrict__ colrange, int grid, int p, ssr_view dimg,
                                                              long total, input_args a) {
    const int pp = p * p, gp = grid * p;
    const float* __restrict__ dp = reinterpret_cast<const float*>(dpatch.p) + dpatch.coff;
    float* __restrict__ gi = reinterpret_cast<float*>(dimg.p) + dimg.coff;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % 3);
        const long pix = e / 3;
        const int sx = (int)(pix % W), sy = (int)((pix / W) % H), n = (int)(pix / ((long)W * H));
        const int r0 = max(rowrange[2 * sy], 0), r1 = min(rowrange[2 * sy + 1], gp);
        const int c0 = max(colrange[2 * sx], 0), c1 = min(colrange[2 * sx + 1], gp);
        if (r0 >= r1 || c0 >= c1) continue;
        double s = 0.0;
        for (int dy = r0; dy < r1; ++dy) {
            const int gy = dy / p, py = dy - gy * p;
            for (int dx = c0; dx < c1; ++dx) {
                const int gx = dx / p, px = dx - gx * p;
                s += (double)dp[((long)n * grid * grid + (long)gy * grid + gx) * dpatch.cs + c * pp + py * p + px];
            }
        }
        const float g = (float)(a.normalize ? s / (double)a.std[c] : s);
        gi[pix * dimg.cs + a.perm[c]] += g;
    }
}

// ---------------------------------------------------------------------------------------------- ssr_layernorm_bwd
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);          // butterfly: every lane ends with the same bits
    return v;
}

// one wave per row, lanes as layernorm_kernel (vit.hip): the statistics are recomputed from the saved input exactly as the forward
// forms them.  Everything a lane reads is in registers before its first store: out may alias dy or r.
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(ssr_view x, const float* __restrict__ gamma, ssr_view dy, ssr_view r, ssr_view out,
                                                            int rows, int C, double eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, C4 = C >> 2;
    if (row >= rows) return;                                               // a whole wave leaves; no block-wide barrier below
    const float* xp = reinterpret_cast<const float*>(x.p) + (long)row * x.cs + x.coff;
    const float* dyp = reinterpret_cast<const float*>(dy.p) + (long)row * dy.cs + dy.coff;
    const float* rp = r.p ? reinterpret_cast<const float*>(r.p) + (long)row * r.cs + r.coff : nullptr;
    float* op = reinterpret_cast<float*>(out.p) + (long)row * out.cs + out.coff;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 v[8], g[8], rr[8];
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c4 = lane + 64 * i;
        rr[i] = zero;
        if (c4 < C4) {
            v[i] = *reinterpret_cast<const f32x4*>(xp + 4 * c4);
            g[i] = *reinterpret_cast<const f32x4*>(dyp + 4 * c4);
            if (rp) rr[i] = *reinterpret_cast<const f32x4*>(rp + 4 * c4);
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
    double sg = 0.0, sgx = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double gj = (double)g[i][j] * (double)gm[j], xh = ((double)v[i][j] - mean) * rstd;
                sg += gj;
                sgx += gj * xh;
            }
        }
    }
    const double m1 = wave_sum(sg) / (double)C, m2 = wave_sum(sgx) / (double)C;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c4 = lane + 64 * i;
        if (c4 < C4) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + 4 * c4);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double gj = (double)g[i][j] * (double)gm[j], xh = ((double)v[i][j] - mean) * rstd;
                const float dx = (float)(rstd * (gj - m1 - xh * m2));
                o[j] = rp ? dx + rr[i][j] : dx;
            }
            *reinterpret_cast<f32x4*>(op + 4 * c4) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------- activation passes
__device__ __forceinline__ float vit_act_grad(float v, int act) {
    switch (act) {
        case SSR_VIT_ACT_QUICK_GELU: {
            const float s = 1.0f / (1.0f + expf(-1.702f * v));
            return s * (1.0f + 1.702f * v * (1.0f - s));
        }
        case SSR_VIT_ACT_GELU_TANH: {
            const float t = tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v));
            return 0.5f * (1.0f + t) + 0.5f * v * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 0.134145f * v * v);
        }
        case SSR_VIT_ACT_GELU_ERF:
            return 0.5f * (1.0f + erff(v * 0.7071067811865476f)) + v * 0.3989422804014327f * expf(-0.5f * v * v);
        default: return 1.0f;
    }
}

// one thread per float4; g.p == NULL: y = act(pre), else y = g * act'(pre).  y may alias g or pre (same element, same thread).
__global__ __launch_bounds__(256) void act_kernel(ssr_view pre, ssr_view g, ssr_view y, long rows, int C, int act) {
    const int C4 = C >> 2;
    const long total = rows * C4;
    const float* pp = reinterpret_cast<const float*>(pre.p) + pre.coff;
    const float* gp = g.p ? reinterpret_cast<const float*>(g.p) + g.coff : nullptr;
    float* yp = reinterpret_cast<float*>(y.p) + y.coff;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / C4;
        const int c = 4 * (int)(i - row * C4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(pp + row * pre.cs + c);
        f32x4 o;
        if (gp) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(gp + row * g.cs + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = gv[j] * vit_act_grad(v[j], act);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = vit_act(v[j], act);
        }
        *reinterpret_cast<f32x4*>(yp + row * y.cs + c) = o;
    }
}

// ---------------------------------------------------------------------------------------------- ssr_mha_bwd
// With S = q k^T scale, P = softmax(S), dP = dy v^T, delta_i = sum_j P_ij dP_ij, dS = P (dP - delta):
//     dv = P^T dy,   dk = scale dS^T q,   dq = scale dS k.
// Tiles of 64 queries x 64 keys as mha_kernel (vit.hip), plain fp32 FMA.  Thread (tq, tk) of "phase 1" forms the 4 x 4 entries rows
// 4 tq + a, columns tk + 16 b of BOTH S (from sQ, sK) and dP (from sG = dy, sV).
//   mha_bwd_q_kernel   a block owns a query tile.  Pass 1 walks the key tiles for the row statistics, exactly the running maximum
//                      m and sum l of the forward plus the running sum of p dP (rescaled alike), so delta = that / l.  They go to the
//                      workspace st[(n heads + h) Tq + i][3] = (m, 1 / l, delta).  Pass 2 (dq wanted) walks the keys again:
//                      dS into LDS, then thread (row, part) adds dS_ij k_j over j ascending into its D / 4 channels of dq.
//   mha_bwd_kv_kernel  a block owns a key tile and walks the query tiles in order: P and dS into LDS from the saved statistics,
//                      then thread (key, part) adds P_ij dy_i and dS_ij q_i over i ascending into its D / 4 channels of dv and dk.
// Keys past Tk are staged as zeros with S = -inf (P = 0); query rows past Tq are staged as zeros with statistics (0, 0, 0): P = 0.
constexpr int MB_T = 64, MB_LS = MB_T + 1;
template <int D> constexpr int mha_bwd_lds_bytes() { return (4 * MB_T * (D + 4) + 2 * MB_T * MB_LS + 3 * MB_T) * (int)sizeof(float); }

template <int D>
__device__ __forceinline__ void load_tile(float* s, const float* __restrict__ g, int cs, long row0, int t0, int T, int tid) {
    constexpr int LD = D + 4, D4 = D / 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int f = tid; f < MB_T * D4; f += 256) {
        const int row = f / D4, c4 = f - row * D4, t = t0 + row;
        *reinterpret_cast<f32x4*>(s + row * LD + 4 * c4) = t < T ? *reinterpret_cast<const f32x4*>(g + (row0 + t) * cs + 4 * c4) : zero;
    }
}

// acc[a][b] = A[4 tq + a] . B[tk + 16 b] over D channels
template <int D>
__device__ __forceinline__ void dot_4x4(const float* sA, const float* sB, int tq, int tk, float (&acc)[4][4]) {
    constexpr int LD = D + 4;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
#pragma unroll 2
    for (int kk = 0; kk < D; kk += 4) {
        f32x4 qa[4], kb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) qa[a] = *reinterpret_cast<const f32x4*>(sA + (4 * tq + a) * LD + kk);
#pragma unroll
        for (int b = 0; b < 4; ++b) kb[b] = *reinterpret_cast<const f32x4*>(sB + (tk + 16 * b) * LD + kk);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[a][b] = fmaf(qa[a][j], kb[b][j], acc[a][b]);
    }
}

template <int D>
__global__ __launch_bounds__(256) void mha_bwd_q_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, float* __restrict__ st,
                                                        int Tq, int Tk, float scale) {
    constexpr int LD = D + 4, DQ = D / 4;
    extern __shared__ float mb_lds[];
    float* sQ = mb_lds;
    float* sG = sQ + MB_T * LD;
    float* sK = sG + MB_T * LD;
    float* sV = sK + MB_T * LD;
    float* sS = sV + MB_T * LD;
    float* sP = sS + MB_T * MB_LS;
    float* sSt = sP + MB_T * MB_LS;                     // [64][3]
    const int tid = threadIdx.x, n = blockIdx.z, h = blockIdx.y, heads = gridDim.y, q0 = blockIdx.x * MB_T;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    const float* __restrict__ gp = reinterpret_cast<const float*>(dy.p) + dy.coff + h * D;
    load_tile<D>(sQ, qp, q.cs, (long)n * Tq, q0, Tq, tid);
    load_tile<D>(sG, gp, dy.cs, (long)n * Tq, q0, Tq, tid);

    const int tq = tid >> 4, tk = tid & 15;            // phase 1
    const int row = tid >> 2, part = tid & 3;          // row phases
    float acc[4][4];

    // pass 1: the statistics
    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
    for (int kt0 = 0; kt0 < Tk; kt0 += MB_T) {
        __syncthreads();                               // the previous tile's row phase has read sS and sP
        load_tile<D>(sK, kp, k.cs, (long)n * Tk, kt0, Tk, tid);
        load_tile<D>(sV, vp, v.cs, (long)n * Tk, kt0, Tk, tid);
        __syncthreads();
        dot_4x4<D>(sQ, sK, tq, tk, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) sS[(4 * tq + a) * MB_LS + tk + 16 * b] = (kt0 + tk + 16 * b < Tk) ? acc[a][b] * scale : -INFINITY;
        dot_4x4<D>(sG, sV, tq, tk, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) sP[(4 * tq + a) * MB_LS + tk + 16 * b] = acc[a][b];
        __syncthreads();
        {
            const float* srow = sS + row * MB_LS + 16 * part;
            const float* prow = sP + row * MB_LS + 16 * part;
            float mt = srow[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) mt = fmaxf(mt, srow[j]);
            mt = fmaxf(mt, __shfl_xor(mt, 1, 64));
            mt = fmaxf(mt, __shfl_xor(mt, 2, 64));
            const float m_new = fmaxf(m_run, mt);       // finite: the tile holds at least one key
            const float alpha = expf(m_run - m_new);    // first tile: exp(-inf) = 0
            float ps = 0.f, pd = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float p = expf(srow[j] - m_new);
                ps += p;
                pd = fmaf(p, prow[j], pd);
            }
            ps += __shfl_xor(ps, 1, 64);
            ps += __shfl_xor(ps, 2, 64);
            pd += __shfl_xor(pd, 1, 64);
            pd += __shfl_xor(pd, 2, 64);
            l_run = l_run * alpha + ps;
            d_run = d_run * alpha + pd;
            m_run = m_new;
        }
    }
    {
        const bool ok = q0 + row < Tq;
        const float il = ok ? 1.0f / l_run : 0.f, dl = ok ? d_run * il : 0.f, mm = ok ? m_run : 0.f;
        if (part == 0) {
            sSt[3 * row] = mm;
            sSt[3 * row + 1] = il;
            sSt[3 * row + 2] = dl;
            if (ok) {
                float* o = st + (((long)n * heads + h) * Tq + q0 + row) * 3;
                o[0] = mm;
                o[1] = il;
                o[2] = dl;
            }
        }
    }
    if (!dq.p) return;                                  // the whole block: uniform

    // pass 2: dq
    float o[DQ];
#pragma unroll
    for (int c = 0; c < DQ; ++c) o[c] = 0.f;
    for (int kt0 = 0; kt0 < Tk; kt0 += MB_T) {
        __syncthreads();                               // sSt written; the previous tile's sums have read sS and sK
        load_tile<D>(sK, kp, k.cs, (long)n * Tk, kt0, Tk, tid);
        load_tile<D>(sV, vp, v.cs, (long)n * Tk, kt0, Tk, tid);
        __syncthreads();
        float dp[4][4];
        dot_4x4<D>(sG, sV, tq, tk, dp);
        dot_4x4<D>(sQ, sK, tq, tk, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float mm = sSt[3 * (4 * tq + a)], il = sSt[3 * (4 * tq + a) + 1], dl = sSt[3 * (4 * tq + a) + 2];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float s = (kt0 + tk + 16 * b < Tk) ? acc[a][b] * scale : -INFINITY;
                const float p = expf(s - mm) * il;
                sS[(4 * tq + a) * MB_LS + tk + 16 * b] = p * (dp[a][b] - dl);
            }
        }
        __syncthreads();
        {
            const float* drow = sS + row * MB_LS;
            const float* kcol = sK + part * DQ;
            for (int j = 0; j < MB_T; ++j) {
                const float ds = drow[j];
#pragma unroll
                for (int c = 0; c < DQ; c += 2) {
                    const float2 kk = *reinterpret_cast<const float2*>(kcol + j * LD + c);
                    o[c] = fmaf(ds, kk.x, o[c]);
                    o[c + 1] = fmaf(ds, kk.y, o[c + 1]);
                }
            }
        }
    }
    const int t = q0 + row;
    if (t < Tq) {
        float* op = reinterpret_cast<float*>(dq.p) + ((long)n * Tq + t) * dq.cs + dq.coff + h * D + part * DQ;
#pragma unroll
        for (int c = 0; c < DQ; c += 2) {
            float2 ov;
            ov.x = o[c] * scale;
            ov.y = o[c + 1] * scale;
            *reinterpret_cast<float2*>(op + c) = ov;
        }
    }
}

template <int D>
__global__ __launch_bounds__(256) void mha_bwd_kv_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dk, ssr_view dv,
                                                         const float* __restrict__ st, int Tq, int Tk, float scale) {
    constexpr int LD = D + 4, DQ = D / 4;
    extern __shared__ float mb_lds[];
    float* sQ = mb_lds;
    float* sG = sQ + MB_T * LD;
    float* sK = sG + MB_T * LD;
    float* sV = sK + MB_T * LD;
    float* sS = sV + MB_T * LD;
    float* sP = sS + MB_T * MB_LS;
    float* sSt = sP + MB_T * MB_LS;
    const int tid = threadIdx.x, n = blockIdx.z, h = blockIdx.y, heads = gridDim.y, k0 = blockIdx.x * MB_T;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    const float* __restrict__ gp = reinterpret_cast<const float*>(dy.p) + dy.coff + h * D;
    load_tile<D>(sK, kp, k.cs, (long)n * Tk, k0, Tk, tid);
    load_tile<D>(sV, vp, v.cs, (long)n * Tk, k0, Tk, tid);

    const int tq = tid >> 4, tk = tid & 15;
    const int key = tid >> 2, part = tid & 3;
    float ok_[DQ], ov_[DQ];
#pragma unroll
    for (int c = 0; c < DQ; ++c) ok_[c] = ov_[c] = 0.f;

    for (int qt0 = 0; qt0 < Tq; qt0 += MB_T) {
        __syncthreads();                               // the previous tile's sums have read sQ, sG, sS and sP
        load_tile<D>(sQ, qp, q.cs, (long)n * Tq, qt0, Tq, tid);
        load_tile<D>(sG, gp, dy.cs, (long)n * Tq, qt0, Tq, tid);
        if (tid < 3 * MB_T) {
            const int r = tid / 3;
            sSt[tid] = qt0 + r < Tq ? st[(((long)n * heads + h) * Tq + qt0) * 3 + tid] : 0.f;
        }
        __syncthreads();
        float acc[4][4], dp[4][4];
        dot_4x4<D>(sG, sV, tq, tk, dp);
        dot_4x4<D>(sQ, sK, tq, tk, acc);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float mm = sSt[3 * (4 * tq + a)], il = sSt[3 * (4 * tq + a) + 1], dl = sSt[3 * (4 * tq + a) + 2];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const float s = (k0 + tk + 16 * b < Tk) ? acc[a][b] * scale : -INFINITY;
                const float p = expf(s - mm) * il;
                sP[(4 * tq + a) * MB_LS + tk + 16 * b] = p;
                sS[(4 * tq + a) * MB_LS + tk + 16 * b] = p * (dp[a][b] - dl);
            }
        }
        __syncthreads();
        for (int i = 0; i < MB_T; ++i) {
            const float p = sP[i * MB_LS + key], ds = sS[i * MB_LS + key];
            const float* grow = sG + i * LD + part * DQ;
            const float* qrow = sQ + i * LD + part * DQ;
#pragma unroll
            for (int c = 0; c < DQ; c += 2) {
                const float2 gg = *reinterpret_cast<const float2*>(grow + c), qq = *reinterpret_cast<const float2*>(qrow + c);
                ov_[c] = fmaf(p, gg.x, ov_[c]);
                ov_[c + 1] = fmaf(p, gg.y, ov_[c + 1]);
                ok_[c] = fmaf(ds, qq.x, ok_[c]);
                ok_[c + 1] = fmaf(ds, qq.y, ok_[c + 1]);
            }
        }
    }
    const int t = k0 + key;
    if (t < Tk) {
        float* kq = reinterpret_cast<float*>(dk.p) + ((long)n * Tk + t) * dk.cs + dk.coff + h * D + part * DQ;
        float* vq = reinterpret_cast<float*>(dv.p) + ((long)n * Tk + t) * dv.cs + dv.coff + h * D + part * DQ;
#pragma unroll
        for (int c = 0; c < DQ; c += 2) {
            float2 a, b;
            a.x = ok_[c] * scale;
            a.y = ok_[c + 1] * scale;
            b.x = ov_[c];
            b.y = ov_[c + 1];
            *reinterpret_cast<float2*>(kq + c) = a;
            *reinterpret_cast<float2*>(vq + c) = b;
        }
    }
}

template <int D>
int launch_mha_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws, int N, int Tq, int Tk,
                   int heads, float scale, hipStream_t st) {
    auto kq = mha_bwd_q_kernel<D>;
    auto kkv = mha_bwd_kv_kernel<D>;
    constexpr int lds = mha_bwd_lds_bytes<D>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr_done[SSR_MAX_DEVICES] = {};      // the attribute is per DEVICE
    const int dev = ssr_device_ordinal();
    if (!attr_done[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kq), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kkv), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        attr_done[dev] = true;
    }
    hipLaunchKernelGGL(kq, dim3((Tq + MB_T - 1) / MB_T, heads, N), dim3(256), lds, st, q, k, v, dy, dq, ws, Tq, Tk, scale);
    hipLaunchKernelGGL(kkv, dim3((Tk + MB_T - 1) / MB_T, heads, N), dim3(256), lds, st, q, k, v, dy, dk, dv, ws, Tq, Tk, scale);
    return 0;
}

// ---------------------------------------------------------------------------------------------- ssr_feature_l1
// one block: 256 elements at a time, every thread writes its element's gradient and stages |fx - fg| as a double in LDS, then thread 0
// alone adds the 256 staged values in index order: ONE fp64 chain over all B * E elements, the memory latency taken in parallel
__global__ __launch_bounds__(256) void feature_l1_kernel(ssr_view fx, ssr_view fg, ssr_view dfx, int B, int E, float weight, float* loss) {
    __shared__ double sabs[256];
    const float* __restrict__ a = reinterpret_cast<const float*>(fx.p) + fx.coff;
    const float* __restrict__ b = reinterpret_cast<const float*>(fg.p) + fg.coff;
    float* __restrict__ g = dfx.p ? reinterpret_cast<float*>(dfx.p) + dfx.coff : nullptr;
    const long total = (long)B * E;
    const float w = weight / (float)total;
    double s = 0.0;
    for (long i0 = 0; i0 < total; i0 += 256) {
        const long i = i0 + threadIdx.x;
        double ad = 0.0;
        if (i < total) {
            const long r = i / E;
            const int c = (int)(i - r * E);
            const float x = a[r * fx.cs + c], z = b[r * fg.cs + c];
            const float d = x - z;
            if (g) g[r * dfx.cs + c] = d > 0.f ? w : d < 0.f ? -w : d == 0.f ? 0.f : d;       // sign(0) = 0; a NaN stays one
            ad = fabs((double)x - (double)z);
        }
        sabs[threadIdx.x] = ad;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = (int)(total - i0 < 256 ? total - i0 : 256);
            for (int j = 0; j < n; ++j) s += sabs[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] += (float)((double)weight * (s / (double)total));
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define VIT_F32(dtype)                           \
    do {                                         \
        if (dtype == SSR_F32X3) dtype = SSR_F32; \
        if (dtype == SSR_BF16) return SSR_EUNSUP;\
        if (dtype != SSR_F32) return SSR_EINVAL; \
    } while (0)

static int input_args_from(const int32_t* perm, const float* mean, const float* std, input_args* a) {
    if (!perm || (mean == nullptr) != (std == nullptr)) return SSR_EINVAL;
    int seen = 0;
    for (int c = 0; c < 3; ++c) {
        if (perm[c] < 0 || perm[c] > 2) return SSR_EINVAL;
        if (mean && !(std[c] != 0.f)) return SSR_EINVAL;
        seen |= 1 << perm[c];
        a->perm[c] = perm[c];
        a->mean[c] = mean ? mean[c] : 0.f;
        a->std[c] = mean ? std[c] : 1.f;
    }
    if (seen != 7) return SSR_EINVAL;                  // a permutation: the backward has one writer per element
    a->normalize = mean ? 1 : 0;
    return SSR_OK;
}

// an fp32 NHWC image view: at least 3 channels, 4-byte aligned (any channel count)
static bool image_view_ok(const ssr_view& v) { return v.p && v.coff >= 0 && v.cs >= v.coff + 3 && !(reinterpret_cast<uintptr_t>(v.p) & 3); }

extern "C" int ssr_vit_float_input(ssr_view img, int32_t N, int32_t H, int32_t W, const int32_t* rowidx, const int32_t* colidx,
                                   int32_t grid, int32_t p, ssr_view y, int32_t dtype, const int32_t* perm, const float* mean,
                                   const float* std, void* stream) {
    VIT_F32(dtype);
    if (!rowidx || !colidx || N <= 0 || H <= 0 || W <= 0 || grid <= 0 || p <= 0) return SSR_EINVAL;
    if (p > 64 || grid > 1024) return SSR_EUNSUP;
    if (!image_view_ok(img) || !view_ok(y, 3 * p * p)) return SSR_EINVAL;
    input_args a;
    if (int rc = input_args_from(perm, mean, std, &a)) return rc;
    const long total = (long)N * grid * grid * 3 * p * p;
    hipLaunchKernelGGL(float_input_kernel, dim3(grid_for(total)), dim3(256), 0, ST(stream), img, H, W, rowidx, colidx, grid, p, y, total, a);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_vit_float_input_bwd(ssr_view dpatch, int32_t N, int32_t H, int32_t W, const int32_t* rowrange, const int32_t* colrange,
                                       int32_t grid, int32_t p, ssr_view dimg, int32_t dtype, const int32_t* perm, const float* std,
                                       void* stream) {
    VIT_F32(dtype);
    if (!rowrange || !colrange || N <= 0 || H <= 0 || W <= 0 || grid <= 0 || p <= 0) return SSR_EINVAL;
    if (p > 64 || grid > 1024) return SSR_EUNSUP;
    if (!image_view_ok(dimg) || !view_ok(dpatch, 3 * p * p)) return SSR_EINVAL;
    input_args a;
    const float zero3[3] = {0.f, 0.f, 0.f};
    if (int rc = input_args_from(perm, std ? zero3 : nullptr, std, &a)) return rc;
    const long total = (long)N * H * W * 3;
    hipLaunchKernelGGL(float_input_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, ST(stream), dpatch, H, W, rowrange, colrange, grid, p,
                       dimg, total, a);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_layernorm_bwd(ssr_view x, const float* gamma, ssr_view dy, ssr_view r, ssr_view out, int32_t dtype, int32_t rows,
                                 int32_t C, double eps, void* stream) {
    VIT_F32(dtype);
    if (rows <= 0 || C <= 0 || !gamma || !(eps >= 0.0)) return SSR_EINVAL;
    if ((C % 4) || C > 2048) return SSR_EUNSUP;
    if (!view_ok(x, C) || !view_ok(dy, C) || !view_ok(out, C) || !aligned16(gamma) || (r.p && !view_ok(r, C))) return SSR_EINVAL;
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, ST(stream), x, gamma, dy, r, out, rows, C, eps);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

static int act_pass(ssr_view pre, ssr_view g, ssr_view y, int32_t dtype, int32_t rows, int32_t C, int32_t act, bool bwd, void* stream) {
    VIT_F32(dtype);
    if (rows <= 0 || C <= 0) return SSR_EINVAL;
    if (act < SSR_VIT_ACT_NONE || act > SSR_VIT_ACT_GELU_ERF) return SSR_EINVAL;
    if (C % 4) return SSR_EUNSUP;
    if (!view_ok(pre, C) || !view_ok(y, C) || (bwd && !view_ok(g, C))) return SSR_EINVAL;
    const ssr_view none = {nullptr, 0, 0};
    hipLaunchKernelGGL(act_kernel, dim3(grid_for((long)rows * (C / 4))), dim3(256), 0, ST(stream), pre, bwd ? g : none, y, (long)rows, C, act);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_vit_act_fwd(ssr_view pre, ssr_view post, int32_t dtype, int32_t rows, int32_t C, int32_t act, void* stream) {
    const ssr_view none = {nullptr, 0, 0};
    return act_pass(pre, none, post, dtype, rows, C, act, false, stream);
}

extern "C" int ssr_vit_act_bwd(ssr_view pre, ssr_view dpost, ssr_view dpre, int32_t dtype, int32_t rows, int32_t C, int32_t act,
                               void* stream) {
    return act_pass(pre, dpost, dpre, dtype, rows, C, act, true, stream);
}

extern "C" int64_t ssr_mha_bwd_ws_floats(int32_t N, int32_t Tq, int32_t heads) {
    if (N <= 0 || Tq <= 0 || heads <= 0) return SSR_EINVAL;
    return 3 * (int64_t)N * heads * Tq;
}

extern "C" int ssr_mha_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws, int32_t dtype,
                           int32_t N, int32_t Tq, int32_t Tk, int32_t heads, int32_t d, float scale, void* stream) {
    VIT_F32(dtype);
    if (N <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || !(scale == scale) || !ws || (reinterpret_cast<uintptr_t>(ws) & 3))
        return SSR_EINVAL;
    if ((d != 64 && d != 72) || N > 65535 || heads > 65535 || Tq > (1 << 20) || Tk > (1 << 20)) return SSR_EUNSUP;
    const int C = heads * d;
    if (!view_ok(q, C) || !view_ok(k, C) || !view_ok(v, C) || !view_ok(dy, C) || !view_ok(dk, C) || !view_ok(dv, C)) return SSR_EINVAL;
    if (dq.p && !view_ok(dq, C)) return SSR_EINVAL;
    const hipStream_t st = ST(stream);
    const int rc = d == 64 ? launch_mha_bwd<64>(q, k, v, dy, dq, dk, dv, ws, N, Tq, Tk, heads, scale, st)
                           : launch_mha_bwd<72>(q, k, v, dy, dq, dk, dv, ws, N, Tq, Tk, heads, scale, st);
    if (rc) return rc;
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_feature_l1(ssr_view fx, ssr_view fg, ssr_view dfx, int32_t B, int32_t E, float weight, float* loss, int32_t flags,
                              void* stream) {
    if (flags != 0 && flags != SSR_DETERMINISTIC) return SSR_EINVAL;      // one block, one writer: slot 0 either way
    if (B <= 0 || E <= 0 || !loss || (reinterpret_cast<uintptr_t>(loss) & 3) || !(weight == weight)) return SSR_EINVAL;
    auto ok = [&](const ssr_view& w) { return w.p && w.coff >= 0 && w.cs >= w.coff + E && !(reinterpret_cast<uintptr_t>(w.p) & 3); };
    if (!ok(fx) || !ok(fg) || (dfx.p && !ok(dfx))) return SSR_EINVAL;
    if ((long)B * E > (1 << 24)) return SSR_EUNSUP;
    hipLaunchKernelGGL(feature_l1_kernel, dim3(1), dim3(256), 0, ST(stream), fx, fg, dfx, B, E, weight, loss);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
