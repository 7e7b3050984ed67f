// What lies between the convolutions of L2Model's networks, SRCNN and HighResNet (include/ssr_hip.h, "L2Model's networks"):
//
//   ssr_prelu_reflect_fwd   PReLU (learned slope, read on the device), Dropout(0.5) from packed keep bits, the residual add, and the
//                           write into the NEXT layer's reflect-padded buffer - interior and border in one launch, optionally into a
//                           channel slice of another image (the revisit -> channel views; no concat is materialised).
//   ssr_prelu_reflect_bwd   the transpose: fold the border gradient back onto the interior, add the residual branch, dropout, PReLU',
//                           and d loss / d slope as per-block fp64 partials + a fixed-order finish.
//   ssr_sr_tail_fwd / _bwd  PixelShuffle + 1x1 conv + PReLU + 1x1 conv + PReLU as one VALU kernel per direction.
//   ssr_dropout_mask        Philox4x32-10 keep bits, the step counter on the device.
//   ssr_mse_l1_loss         both pixel terms of L2Model's loss and their combined gradient in one pass.
//
// All of them stream: one thread per 16-byte channel vector (the tail: per output pixel), no LDS except the block reductions, no
// float atomics anywhere - two launches on the same inputs give the same bytes.  Products that torch rounds separately are kept
// apart from the adds behind them (__fmul_rn / __fadd_rn): the forward and the data gradient are bit-exact fp32 restatements.
#include "common.h"

namespace {

constexpr int BLK = 256;

__device__ __forceinline__ int reflect_idx(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

inline bool view4_ok(const ssr_view& v, int need) {
    return v.p && v.cs > 0 && v.coff >= 0 && (v.cs % 4) == 0 && (v.coff % 4) == 0 && v.coff + need <= v.cs &&
           (reinterpret_cast<uintptr_t>(v.p) % 16) == 0;
}

// block-wide sum of doubles in a fixed order (lane order inside a wave by xor-shuffles, then the waves in index order)
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sh[w];
    return s;
}

// ------------------------------------------------------------------------------------------------ PReLU / dropout / reflect
// one thread per (padded output pixel, 4-channel vector): a border pixel recomputes the interior sample it reflects
__global__ __launch_bounds__(BLK) void prelu_reflect_fwd_kernel(const ssr_prelu_reflect_desc d) {
    const int C4 = d.C >> 2, P = d.out_pad, HP = d.H + 2 * P, WP = d.W + 2 * P;
    const long total = (long)d.N * HP * WP * C4;
    const float a = d.slope[0];
    const float* __restrict__ pre = reinterpret_cast<const float*>(d.pre.p);
    const float* __restrict__ res = reinterpret_cast<const float*>(d.res.p);
    float* __restrict__ out = reinterpret_cast<float*>(d.out.p);
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < total; i += (long)gridDim.x * BLK) {
        long t = i;
        const int c = (int)(t % C4) * 4; t /= C4;
        const int px = (int)(t % WP); t /= WP;
        const int py = (int)(t % HP);
        const int n = (int)(t / HP);
        const int y = reflect_idx(py - P, d.H), x = reflect_idx(px - P, d.W);
        const long e = (((long)n * d.H + y) * d.W + x);
        f32x4 v = *reinterpret_cast<const f32x4*>(pre + e * d.pre.cs + d.pre.coff + c);
        uint32_t keep = 0xfu;
        if (d.mask) {
            const long eb = e * d.C + c;                       // multiple of 4: the four bits lie in one word
            keep = (d.mask[eb >> 5] >> (eb & 31)) & 0xfu;
        }
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (res) {
            const long rp = ((long)n * (d.H + 2 * d.res_pad) + y + d.res_pad) * (d.W + 2 * d.res_pad) + x + d.res_pad;
            r = *reinterpret_cast<const f32x4*>(res + rp * d.res.cs + d.res.coff + c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float s = v[k] > 0.f ? v[k] : __fmul_rn(a, v[k]);
            if (d.mask) s = ((keep >> k) & 1u) ? __fmul_rn(s, 2.f) : 0.f;
            if (res) s = __fadd_rn(r[k], s);
            v[k] = s;
        }
        const int b = n / d.group, rr = n - b * d.group;
        const long on = (long)b * d.fold + rr % d.fold;
        const long op = (on * HP + py) * WP + px;
        *reinterpret_cast<f32x4*>(out + op * d.out.cs + d.out.coff + (rr / d.fold) * d.C + c) = v;
    }
}

// fold of one gradient buffer onto interior pixel (y, x): rows, then columns, in increasing padded index
__device__ __forceinline__ void fold_add(f32x4& acc, bool& first, const float* __restrict__ g, const ssr_view& gv, int pad, long img,
                                         int y, int x, int H, int W, int coff) {
    if (!pad) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(g + ((img * H + y) * W + x) * gv.cs + coff);
        if (first) { acc = v; first = false; }
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], v[k]);
        }
        return;
    }
    const int HP = H + 2, WP = W + 2;
    // padded rows that read interior row y: 0 (if y == 1), y + 1, H + 1 (if y == H - 2), in increasing order
    int rows[3], cols[3], nr = 0, nc = 0;
    if (y == 1) rows[nr++] = 0;
    rows[nr++] = y + 1;
    if (y == H - 2) rows[nr++] = H + 1;
    if (x == 1) cols[nc++] = 0;
    cols[nc++] = x + 1;
    if (x == W - 2) cols[nc++] = W + 1;
    for (int a = 0; a < nr; ++a)
        for (int b = 0; b < nc; ++b) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(g + ((img * HP + rows[a]) * WP + cols[b]) * gv.cs + coff);
            if (first) { acc = v; first = false; }
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], v[k]);
            }
        }
}

__global__ __launch_bounds__(BLK) void prelu_reflect_bwd_kernel(const ssr_prelu_reflect_desc d) {
    __shared__ double sh[BLK / 64];
    const int C4 = d.C >> 2;
    const long total = (long)d.N * d.H * d.W * C4;
    const float a = d.slope[0];
    const float* __restrict__ pre = reinterpret_cast<const float*>(d.pre.p);
    const float* __restrict__ g = reinterpret_cast<const float*>(d.g.p);
    const float* __restrict__ g2 = reinterpret_cast<const float*>(d.g2.p);
    float* __restrict__ dpre = reinterpret_cast<float*>(d.dpre.p);
    double part = 0.0;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < total; i += (long)gridDim.x * BLK) {
        long t = i;
        const int c = (int)(t % C4) * 4; t /= C4;
        const int x = (int)(t % d.W); t /= d.W;
        const int y = (int)(t % d.H);
        const int n = (int)(t / d.H);
        const long e = (((long)n * d.H + y) * d.W + x);
        const int b = n / d.group, rr = n - b * d.group;
        const long img = (long)b * d.fold + rr % d.fold;
        const int cm = (rr / d.fold) * d.C + c;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        bool first = true;
        fold_add(acc, first, g, d.g, d.g_pad, img, y, x, d.H, d.W, d.g.coff + cm);
        if (g2) fold_add(acc, first, g2, d.g2, d.g2_pad, img, y, x, d.H, d.W, d.g2.coff + cm);
        const f32x4 v = *reinterpret_cast<const f32x4*>(pre + e * d.pre.cs + d.pre.coff + c);
        uint32_t keep = 0xfu;
        if (d.mask) {
            const long eb = e * d.C + c;
            keep = (d.mask[eb >> 5] >> (eb & 31)) & 0xfu;
        }
        if (d.tsum.p) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(d.tsum.p) + e * d.tsum.cs + d.tsum.coff + c) = acc;
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float tk = acc[k];
            if (d.mask) tk = ((keep >> k) & 1u) ? __fmul_rn(tk, 2.f) : 0.f;
            o[k] = v[k] > 0.f ? tk : __fmul_rn(a, tk);
            if (!(v[k] > 0.f)) part += (double)v[k] * (double)tk;
        }
        *reinterpret_cast<f32x4*>(dpre + e * d.dpre.cs + d.dpre.coff + c) = o;
    }
    const double s = block_sum(part, sh);
    if (threadIdx.x == 0) d.partial[blockIdx.x] = s;
}

// dst[k] += sum over the blocks of partial[b * stride + k], one wave per k: lane l adds the slots l, l + 64, .. in that order, the
// 64 lane sums meet in a butterfly - a fixed order whatever the blocks' finishing order was
__global__ __launch_bounds__(64) void finish_partials_kernel(const double* __restrict__ partial, int nblk, int stride, float* dst) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) s += partial[(long)b * stride + k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) dst[k] = __fadd_rn(dst[k], (float)s);
}

// ------------------------------------------------------------------------------------------------ dropout keep bits
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* o) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__global__ __launch_bounds__(BLK) void dropout_mask_kernel(uint32_t* __restrict__ bits, long n4, uint32_t k0, uint32_t k1,
                                                           const int32_t* __restrict__ step, uint32_t layer) {
    const uint32_t st = (uint32_t)step[0];
    for (long j = (long)blockIdx.x * BLK + threadIdx.x; j < n4; j += (long)gridDim.x * BLK) {
        uint32_t o[4];
        philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), st, layer, k0, k1, o);
        u32x4 w = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<u32x4*>(bits + 4 * j) = w;
    }
}
__global__ void bump_step_kernel(int32_t* step) { step[0] += 1; }

// ------------------------------------------------------------------------------------------------ PixelShuffle tail
constexpr int CM_MAX = 32, CO_MAX = 8, TAIL_SLOTS = 128, TAIL_CHUNK = 64;

// CMT: compile-time bound of Cm (2, 8 or 32) so that the per-pixel vectors stay in registers
template <int CMT> struct TailPix {
    float u[CMT], p1[CMT], a1[CMT], p2[CO_MAX];
};

template <int CMT>
__device__ __forceinline__ void tail_forward(const ssr_sr_tail_desc& d, int Cm, long pix, TailPix<CMT>& t, long& xoff) {
    const int z = d.zoom, WO = d.W * z, HO = d.H * z;
    const int X = (int)(pix % WO);
    const int Y = (int)((pix / WO) % HO);
    const int n = (int)(pix / ((long)WO * HO));
    const int y = Y / z, x = X / z, sub = (Y - y * z) * z + (X - x * z);
    xoff = (((long)n * d.H + y) * d.W + x) * d.x.cs + d.x.coff + sub;
    const float* __restrict__ xp = reinterpret_cast<const float*>(d.x.p) + xoff;
    const int zz = z * z;
#pragma unroll
    for (int c = 0; c < CMT; ++c) t.u[c] = c < Cm ? xp[c * zz] : 0.f;
    const float s1 = d.s1[0];
#pragma unroll
    for (int k = 0; k < CMT; ++k) {
        float acc = 0.f;
        if (k < Cm) {
            acc = d.b1[k];
#pragma unroll
            for (int c = 0; c < CMT; ++c)
                if (c < Cm) acc = fmaf(d.w1[k * Cm + c], t.u[c], acc);
        }
        t.p1[k] = acc;
        t.a1[k] = acc > 0.f ? acc : s1 * acc;
    }
#pragma unroll
    for (int o = 0; o < CO_MAX; ++o) {
        float acc = 0.f;
        if (o < d.Cout) {
            acc = d.b2[o];
#pragma unroll
            for (int k = 0; k < CMT; ++k)
                if (k < Cm) acc = fmaf(d.w2[o * Cm + k], t.a1[k], acc);
        }
        t.p2[o] = acc;
    }
}

template <int CMT>
__global__ __launch_bounds__(BLK) void sr_tail_fwd_kernel(const ssr_sr_tail_desc d, int Cm, long npix) {
    float* __restrict__ yp = reinterpret_cast<float*>(d.y.p);
    const float s2 = d.s2[0];
    for (long pix = (long)blockIdx.x * BLK + threadIdx.x; pix < npix; pix += (long)gridDim.x * BLK) {
        TailPix<CMT> t;
        long xoff;
        tail_forward<CMT>(d, Cm, pix, t, xoff);
#pragma unroll
        for (int o = 0; o < CO_MAX; ++o)
            if (o < d.Cout) yp[pix * d.y.cs + d.y.coff + o] = t.p2[o] > 0.f ? t.p2[o] : s2 * t.p2[o];
    }
}

// scratch row of one output pixel: [u (Cm) | dp1 (Cm) | a1 (Cm) | dp2 (Cout) | t1 | t2]
__device__ __host__ inline int tail_row(int Cm, int Cout) { return 3 * Cm + Cout + 2; }
__device__ __host__ inline int tail_params(int Cm, int Cout) { return Cm * Cm + Cm + 1 + Cout * Cm + Cout + 1; }

template <int CMT>
__global__ __launch_bounds__(BLK) void sr_tail_bwd_data_kernel(const ssr_sr_tail_desc d, int Cm, long npix, float* __restrict__ rows) {
    const float* __restrict__ gy = reinterpret_cast<const float*>(d.gy.p);
    float* __restrict__ dx = reinterpret_cast<float*>(d.dx.p);
    const float s1 = d.s1[0], s2 = d.s2[0];
    const int R = tail_row(Cm, d.Cout), zz = d.zoom * d.zoom;
    for (long pix = (long)blockIdx.x * BLK + threadIdx.x; pix < npix; pix += (long)gridDim.x * BLK) {
        TailPix<CMT> t;
        long xoff;
        tail_forward<CMT>(d, Cm, pix, t, xoff);
        float* __restrict__ row = rows + pix * R;
        float dp2[CO_MAX];
        float t2 = 0.f;
#pragma unroll
        for (int o = 0; o < CO_MAX; ++o) {
            dp2[o] = 0.f;
            if (o < d.Cout) {
                const float g = gy[pix * d.gy.cs + d.gy.coff + o];
                const bool pos = t.p2[o] > 0.f;
                dp2[o] = pos ? g : s2 * g;
                if (!pos) t2 += t.p2[o] * g;
                row[3 * Cm + o] = dp2[o];
            }
        }
        float t1 = 0.f;
        float dp1[CMT];
#pragma unroll
        for (int k = 0; k < CMT; ++k) {
            dp1[k] = 0.f;
            if (k < Cm) {
                float da = 0.f;
#pragma unroll
                for (int o = 0; o < CO_MAX; ++o)
                    if (o < d.Cout) da = fmaf(d.w2[o * Cm + k], dp2[o], da);
                const bool pos = t.p1[k] > 0.f;
                dp1[k] = pos ? da : s1 * da;
                if (!pos) t1 += t.p1[k] * da;
                row[Cm + k] = dp1[k];
                row[2 * Cm + k] = t.a1[k];
                row[k] = t.u[k];
            }
        }
        row[3 * Cm + d.Cout] = t1;
        row[3 * Cm + d.Cout + 1] = t2;
        // dx in the unshuffled layout: the (pixel, c) -> element map is a bijection, every element is written once
        const long dxoff = xoff - d.x.coff + d.dx.coff;          // same pixel and sub-position (dx.cs == x.cs)
#pragma unroll
        for (int c = 0; c < CMT; ++c) {
            if (c < Cm) {
                float du = 0.f;
#pragma unroll
                for (int k = 0; k < CMT; ++k)
                    if (k < Cm) du = fmaf(d.w1[k * Cm + c], dp1[k], du);
                dx[dxoff + (long)c * zz] = du;
            }
        }
    }
}

// parameter p of [dw1 | db1 | ds1 | dw2 | db2 | ds2] as a product of two entries of a scratch row (ib < 0: times one)
__device__ __forceinline__ void tail_param_index(int p, int Cm, int Cout, int& ia, int& ib) {
    if (p < Cm * Cm) { ia = Cm + p / Cm; ib = p % Cm; return; }
    p -= Cm * Cm;
    if (p < Cm) { ia = Cm + p; ib = -1; return; }
    p -= Cm;
    if (p < 1) { ia = 3 * Cm + Cout; ib = -1; return; }
    p -= 1;
    if (p < Cout * Cm) { ia = 3 * Cm + p / Cm; ib = 2 * Cm + p % Cm; return; }
    p -= Cout * Cm;
    if (p < Cout) { ia = 3 * Cm + p; ib = -1; return; }
    ia = 3 * Cm + Cout + 1; ib = -1;
}

constexpr int TAIL_PPT = 6;      // parameters per thread: CM_MAX^2 + ... <= 6 * 256
__global__ __launch_bounds__(BLK) void sr_tail_bwd_param_kernel(const float* __restrict__ rows, long npix, int Cm, int Cout, int nblk,
                                                                double* __restrict__ partial) {
    extern __shared__ float lds[];                                  // TAIL_CHUNK rows
    const int R = tail_row(Cm, Cout), P = tail_params(Cm, Cout);
    const long per = (npix + nblk - 1) / nblk;
    const long p0 = (long)blockIdx.x * per, p1 = p0 + per < npix ? p0 + per : npix;
    int ia[TAIL_PPT], ib[TAIL_PPT];
    double acc[TAIL_PPT];
#pragma unroll
    for (int q = 0; q < TAIL_PPT; ++q) {
        acc[q] = 0.0;
        ia[q] = ib[q] = -1;
        const int p = threadIdx.x + q * BLK;
        if (p < P) tail_param_index(p, Cm, Cout, ia[q], ib[q]);
    }
    for (long c0 = p0; c0 < p1; c0 += TAIL_CHUNK) {
        const int np = (int)(p1 - c0 < TAIL_CHUNK ? p1 - c0 : TAIL_CHUNK);
        __syncthreads();
        for (int v = threadIdx.x; v < np * R; v += BLK) lds[v] = rows[c0 * R + v];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < TAIL_PPT; ++q) {
            if (ia[q] < 0) continue;
            for (int j = 0; j < np; ++j) {
                const float* r = lds + j * R;
                acc[q] += ib[q] >= 0 ? (double)r[ia[q]] * (double)r[ib[q]] : (double)r[ia[q]];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < TAIL_PPT; ++q) {
        const int p = threadIdx.x + q * BLK;
        if (p < P) partial[(long)blockIdx.x * P + p] = acc[q];
    }
}

struct TailDst { float* p[6]; int n[6]; };
__global__ void sr_tail_finish_kernel(const double* __restrict__ partial, int nblk, int P, const TailDst dst) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= P) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partial[(long)b * P + k];
    int seg = 0;
    while (k >= dst.n[seg]) { k -= dst.n[seg]; ++seg; }
    dst.p[seg][k] = __fadd_rn(dst.p[seg][k], (float)s);
}

inline int tail_blocks(long npix) {
    const long b = (npix + TAIL_CHUNK - 1) / TAIL_CHUNK;
    return (int)(b < TAIL_SLOTS ? b : TAIL_SLOTS);
}

inline int tail_check(const ssr_sr_tail_desc* d, int& Cm) {
    if (!d) return SSR_EINVAL;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->hidden <= 0 || d->zoom <= 0 || d->Cout <= 0) return SSR_EINVAL;
    const int zz = d->zoom * d->zoom;
    if (d->hidden % zz) return SSR_EINVAL;
    Cm = d->hidden / zz;
    if (!d->x.p || d->x.cs <= 0 || d->x.coff < 0 || d->x.coff + d->hidden > d->x.cs) return SSR_EINVAL;
    if (!d->w1 || !d->b1 || !d->s1 || !d->w2 || !d->b2 || !d->s2) return SSR_EINVAL;
    if (Cm > CM_MAX || d->Cout > CO_MAX) return SSR_EUNSUP;
    return SSR_OK;
}

// ------------------------------------------------------------------------------------------------ mse + l1
__global__ __launch_bounds__(BLK) void mse_l1_kernel(ssr_view a, ssr_view b, ssr_view grad, long npix, int C, float cm, float cl,
                                                     double inv_n, double* __restrict__ partial) {
    __shared__ double sh[BLK / 64];
    const float* __restrict__ ap = reinterpret_cast<const float*>(a.p);
    const float* __restrict__ bp = reinterpret_cast<const float*>(b.p);
    float* __restrict__ gp = reinterpret_cast<float*>(grad.p);
    double s2 = 0.0, s1 = 0.0;
    const long total = npix * C;
    for (long i = (long)blockIdx.x * BLK + threadIdx.x; i < total; i += (long)gridDim.x * BLK) {
        const long p = i / C;
        const int c = (int)(i - p * C);
        const float dd = __fsub_rn(ap[p * a.cs + a.coff + c], bp[p * b.cs + b.coff + c]);
        s2 += (double)dd * (double)dd;
        s1 += fabs((double)dd);
        if (gp) gp[p * grad.cs + grad.coff + c] = __fadd_rn(__fmul_rn(cm, dd), dd > 0.f ? cl : (dd < 0.f ? -cl : 0.f));
    }
    const double r2 = block_sum(s2, sh);
    const double r1 = block_sum(s1, sh);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = r2 * inv_n;
        partial[2 * blockIdx.x + 1] = r1 * inv_n;
    }
}

inline int grid_for(long total) {
    const long b = (total + BLK - 1) / BLK;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

inline int prelu_check(const ssr_prelu_reflect_desc* d) {
    if (!d) return SSR_EINVAL;
    if (d->N <= 0 || d->C <= 0 || d->H < 2 || d->W < 2 || (d->C % 4) != 0) return SSR_EINVAL;
    if (d->group < 1 || d->fold < 1 || (d->N % d->group) != 0) return SSR_EINVAL;
    if (!d->slope || !view4_ok(d->pre, d->C)) return SSR_EINVAL;
    if (d->mask && (reinterpret_cast<uintptr_t>(d->mask) % 4) != 0) return SSR_EINVAL;
    return SSR_OK;
}

}  // namespace

extern "C" int ssr_prelu_reflect_fwd(const ssr_prelu_reflect_desc* d, void* stream) {
    int rc = prelu_check(d);
    if (rc) return rc;
    const int slices = (d->group + d->fold - 1) / d->fold;
    if (!view4_ok(d->out, slices * d->C) || (d->out_pad != 0 && d->out_pad != 1)) return SSR_EINVAL;
    if (d->res.p && (!view4_ok(d->res, d->C) || (d->res_pad != 0 && d->res_pad != 1))) return SSR_EINVAL;
    const long total = (long)d->N * (d->H + 2 * d->out_pad) * (d->W + 2 * d->out_pad) * (d->C / 4);
    hipLaunchKernelGGL(prelu_reflect_fwd_kernel, dim3(grid_for(total)), dim3(BLK), 0, (hipStream_t)stream, *d);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_prelu_reflect_bwd(const ssr_prelu_reflect_desc* d, void* stream) {
    int rc = prelu_check(d);
    if (rc) return rc;
    const int slices = (d->group + d->fold - 1) / d->fold;
    if (!view4_ok(d->g, slices * d->C) || (d->g_pad != 0 && d->g_pad != 1)) return SSR_EINVAL;
    if (d->g2.p && (!view4_ok(d->g2, slices * d->C) || (d->g2_pad != 0 && d->g2_pad != 1))) return SSR_EINVAL;
    if (!view4_ok(d->dpre, d->C) || !d->dslope || !d->partial) return SSR_EINVAL;
    if (d->tsum.p && !view4_ok(d->tsum, d->C)) return SSR_EINVAL;
    const long total = (long)d->N * d->H * d->W * (d->C / 4);
    long nb = (total + BLK - 1) / BLK;
    const int nblk = (int)(nb < SSR_L2_SLOTS ? nb : SSR_L2_SLOTS);
    hipLaunchKernelGGL(prelu_reflect_bwd_kernel, dim3(nblk), dim3(BLK), 0, (hipStream_t)stream, *d);
    SSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_partials_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d->partial, nblk, 1, d->dslope);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_dropout_mask(uint32_t* bits, int64_t n_words, uint64_t seed, int32_t* step, int32_t layer, int32_t advance,
                                void* stream) {
    if (!bits || !step || n_words <= 0 || (n_words % 4) != 0 || (reinterpret_cast<uintptr_t>(bits) % 16) != 0) return SSR_EINVAL;
    const long n4 = n_words / 4;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n4)), dim3(BLK), 0, (hipStream_t)stream, bits, n4, (uint32_t)seed,
                       (uint32_t)(seed >> 32), step, (uint32_t)layer);
    SSR_LAUNCH_CHECK();
    if (advance) {
        hipLaunchKernelGGL(bump_step_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
        SSR_LAUNCH_CHECK();
    }
    return SSR_OK;
}

extern "C" int64_t ssr_sr_tail_scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t hidden, int32_t zoom, int32_t Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || hidden <= 0 || zoom <= 0 || Cout <= 0 || hidden % (zoom * zoom)) return SSR_EINVAL;
    const int Cm = hidden / (zoom * zoom);
    const long npix = (long)N * H * W * zoom * zoom;
    long rows = npix * tail_row(Cm, Cout) * 4;
    rows = (rows + 15) / 16 * 16;
    return rows + (long)TAIL_SLOTS * tail_params(Cm, Cout) * 8;
}

extern "C" int ssr_sr_tail_fwd(const ssr_sr_tail_desc* d, void* stream) {
    int Cm = 0;
    int rc = tail_check(d, Cm);
    if (rc) return rc;
    if (!d->y.p || d->y.cs <= 0 || d->y.coff < 0 || d->y.coff + d->Cout > d->y.cs) return SSR_EINVAL;
    const long npix = (long)d->N * d->H * d->W * d->zoom * d->zoom;
    if (Cm <= 2) hipLaunchKernelGGL(sr_tail_fwd_kernel<2>, dim3(grid_for(npix)), dim3(BLK), 0, (hipStream_t)stream, *d, Cm, npix);
    else if (Cm <= 8) hipLaunchKernelGGL(sr_tail_fwd_kernel<8>, dim3(grid_for(npix)), dim3(BLK), 0, (hipStream_t)stream, *d, Cm, npix);
    else hipLaunchKernelGGL(sr_tail_fwd_kernel<CM_MAX>, dim3(grid_for(npix)), dim3(BLK), 0, (hipStream_t)stream, *d, Cm, npix);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_sr_tail_bwd(const ssr_sr_tail_desc* d, void* stream) {
    int Cm = 0;
    int rc = tail_check(d, Cm);
    if (rc) return rc;
    if (!d->gy.p || d->gy.cs <= 0 || d->gy.coff < 0 || d->gy.coff + d->Cout > d->gy.cs) return SSR_EINVAL;
    if (!d->dx.p || d->dx.cs != d->x.cs || d->dx.coff < 0 || d->dx.coff + d->hidden > d->dx.cs) return SSR_EINVAL;
    if (!d->dw1 || !d->db1 || !d->ds1 || !d->dw2 || !d->db2 || !d->ds2 || !d->scratch) return SSR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d->scratch) % 16) != 0) return SSR_EINVAL;
    const long npix = (long)d->N * d->H * d->W * d->zoom * d->zoom;
    const int R = tail_row(Cm, d->Cout), P = tail_params(Cm, d->Cout);
    float* rows = reinterpret_cast<float*>(d->scratch);
    long rbytes = npix * R * 4;
    rbytes = (rbytes + 15) / 16 * 16;
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(d->scratch) + rbytes);
    const int nblk = tail_blocks(npix);
    hipStream_t st = (hipStream_t)stream;
    if (Cm <= 2) hipLaunchKernelGGL(sr_tail_bwd_data_kernel<2>, dim3(grid_for(npix)), dim3(BLK), 0, st, *d, Cm, npix, rows);
    else if (Cm <= 8) hipLaunchKernelGGL(sr_tail_bwd_data_kernel<8>, dim3(grid_for(npix)), dim3(BLK), 0, st, *d, Cm, npix, rows);
    else hipLaunchKernelGGL(sr_tail_bwd_data_kernel<CM_MAX>, dim3(grid_for(npix)), dim3(BLK), 0, st, *d, Cm, npix, rows);
    SSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sr_tail_bwd_param_kernel, dim3(nblk), dim3(BLK), (size_t)TAIL_CHUNK * R * sizeof(float), st, rows, npix, Cm,
                       (int)d->Cout, nblk, partial);
    SSR_LAUNCH_CHECK();
    TailDst dst;
    dst.p[0] = d->dw1; dst.n[0] = Cm * Cm;
    dst.p[1] = d->db1; dst.n[1] = Cm;
    dst.p[2] = d->ds1; dst.n[2] = 1;
    dst.p[3] = d->dw2; dst.n[3] = d->Cout * Cm;
    dst.p[4] = d->db2; dst.n[4] = d->Cout;
    dst.p[5] = d->ds2; dst.n[5] = 1;
    hipLaunchKernelGGL(sr_tail_finish_kernel, dim3((P + BLK - 1) / BLK), dim3(BLK), 0, st, partial, nblk, P, dst);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_mse_l1_loss(ssr_view a, ssr_view b, ssr_view grad, int64_t npix, int32_t C, float w_mse, float w_l1, float* sums,
                               double* partial, void* stream) {
    if (!a.p || !b.p || !sums || !partial || npix <= 0 || C <= 0) return SSR_EINVAL;
    if (a.coff < 0 || b.coff < 0 || a.coff + C > a.cs || b.coff + C > b.cs) return SSR_EINVAL;
    if (grad.p && (grad.coff < 0 || grad.coff + C > grad.cs)) return SSR_EINVAL;
    const double n = (double)npix * (double)C;
    long nb = (npix * C + BLK - 1) / BLK;
    const int nblk = (int)(nb < SSR_L2_SLOTS ? nb : SSR_L2_SLOTS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mse_l1_kernel, dim3(nblk), dim3(BLK), 0, st, a, b, grad, (long)npix, (int)C, (float)(2.0 * w_mse / n),
                       (float)(w_l1 / n), 1.0 / n, partial);
    SSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(finish_partials_kernel, dim3(2), dim3(64), 0, st, partial, nblk, 2, sums);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
