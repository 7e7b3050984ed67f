// The tower's self-attention on the fp32-input matrix core (`tower_attention: mfma` of train.clip_opt and of calculate_clipscore):
// the mathematics of ssr_mha_fwd (vit.hip) and ssr_mha_bwd (vit_bwd.hip) with every matrix product on v_mfma_f32_32x32x2_f32, whose
// result is bit for bit a k-ordered fmaf chain: against the FMA kernels only the order of the additions differs.
//
//   ssr_mha_mfma_fwd   y = softmax(q k^T scale) v per (image, head), keys 64 at a time with a running maximum and sum
//   ssr_mha_mfma_bwd   dS = P (dP - delta): dv = P^T dy, dk = scale dS^T q, dq = scale dS k; statistics recomputed; two owners
//
// One scheme serves all three kernels.  A block of 4 waves OWNS 128 rows of one (image, head): queries in the forward and in the
// backward's query kernel, keys in its key kernel.  Wave w owns rows 32 w .. 32 w + 31, and lanes l and l + 32 (li = l & 31, lg = l >> 5)
// share owned row li: its operands live in their REGISTERS, half of the head dim each (lane half lg holds channels 4 t + 2 lg and
// 4 t + 2 lg + 1, t < D / 4).  The other side is WALKED 64 rows at a time through LDS, one natural [row][D + 2] image per operand.
//
//   product 1 (contracts the head dim)   X[walked][owned] = sum_c W[walked][c] O[owned][c]: the MFMA's A operand is the LDS tile (lane
//       (li, lg) reads W[32 b + li][4 t + 2 lg ..], one ds_read_b64 for two MFMA steps), its B operand the owned registers.  A lane ends
//       with COLUMN = its owned row and the 2 x 16 registers of the walked rows 32 b + mfma32_row(r, lg): everything the softmax needs
//       per owned row (running maximum, sum, delta) is per-lane scalar arithmetic and one exchange with lane l ^ 32.
//   product 2 (contracts the walked rows)   Out^T[c][owned] = sum_w W[w][c] X[w][owned]: X is the B operand straight from the
//       registers product 1 left it in (register r of lane half lg IS walked row mfma32_row(r, lg), which is what k slot lg of the
//       step must supply), the A operand is W[that row][32 cb + li] from the same LDS image.  No P or dS ever goes through LDS.
//       The result has the owned row on the lane again and the output channels 32 cb + mfma32_row(r, lg) in registers: four
//       consecutive channels per register quad, stored as one 16-byte word.
//
// One LDS image serves both reads: product 2 takes 32 consecutive words per lane half, product 1 an 8-byte word at li (D + 2) + 2 lg + 4 t.
// The row stride D + 2 (66 or 74 words, even for the 8-byte reads) is odd in 8-byte units (33, 37), so the 32 rows of product 1 spread
// over all banks instead of meeting in the few a stride of D or D + 4 words would give them.
//
// Head dim 72: product 1 contracts 36 steps of 2, no padding.  In product 2 the head dim is the OUTPUT side: 32 x 32 blocks padded to 96
// (cb = 2 keeps lanes li < 8; the others supply a register zero and their results are never stored).  The alternative, 16 x 16 x 4 blocks
// padded to 80, has another accumulator layout (4 rows per lane quarter), so X could not pass from product 1 to product 2 in registers,
// and its 40-cycle dependent latency wants two chains per wave; the padding costs 96 / 72 on half of the products of one tower family.
//
// Masking is zeros in registers or LDS, never a product with something read: walked rows past T are staged as zeros, owned rows past T
// are zero registers and are not stored; keys past Tk get the logit -inf (p = 0).  Nothing outside the views is touched.
// No atomics, no split reductions: one fixed order of additions per output, the same for every image whatever N.
#include "common.h"
#include <math.h>

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool view_ok(const ssr_view& v, int c) {
    return v.p && v.coff >= 0 && v.cs >= v.coff + c && !(v.cs % 4) && !(v.coff % 4) && aligned16(v.p);
}

constexpr int MM_OWN = 128;     // rows a block owns: 32 per wave
constexpr int MM_TILE = 64;     // walked rows per LDS tile
template <int D> constexpr int mm_ld() { return D + 2; }
template <int D> constexpr int mm_cb() { return (D + 31) / 32; }
template <int D> constexpr int mm_tile_floats() { return MM_TILE * mm_ld<D>(); }

// 64 walked rows t0 .. t0 + 63 of g (row stride cs) -> s[row][D + 2]; rows >= T are zeros and read nothing
template <int D>
__device__ __forceinline__ void stage_tile(float* s, const float* __restrict__ g, int cs, long row0, int t0, int T, int tid) {
    constexpr int LD = mm_ld<D>(), D4 = D / 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int f = tid; f < MM_TILE * D4; f += 256) {
        const int row = f / D4, c4 = f - row * D4, t = t0 + row;
        const f32x4 v = t < T ? *reinterpret_cast<const f32x4*>(g + (row0 + t) * cs + 4 * c4) : zero;
        float2* d = reinterpret_cast<float2*>(s + row * LD + 4 * c4);         // LD is even: 8-byte aligned
        d[0] = make_float2(v[0], v[1]);
        d[1] = make_float2(v[2], v[3]);
    }
}

// the owned row t of g into registers: o[i] = channels 4 i + 2 lg, 4 i + 2 lg + 1; a row >= T is zeros and reads nothing
template <int D>
__device__ __forceinline__ void load_owned(float2 (&o)[D / 4], const float* __restrict__ g, int cs, long row0, int t, int T, int lg) {
#pragma unroll
    for (int i = 0; i < D / 4; ++i)
        o[i] = t < T ? *reinterpret_cast<const float2*>(g + (row0 + t) * cs + 4 * i + 2 * lg) : make_float2(0.f, 0.f);
}

// product 1: x[b][r] = sum_c W[32 b + mfma32_row(r, lg)][c] * owned[c] for this lane's owned row
template <int D>
__device__ __forceinline__ void dot_head(const float* sW, const float2 (&o)[D / 4], int li, int lg, f32x16 (&x)[2]) {
    constexpr int LD = mm_ld<D>();
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) x[b][e] = 0.f;
    const float* w0 = sW + li * LD + 2 * lg;
    const float* w1 = w0 + 32 * LD;
#pragma unroll
    for (int i = 0; i < D / 4; ++i) {
        const float2 a0 = *reinterpret_cast<const float2*>(w0 + 4 * i), a1 = *reinterpret_cast<const float2*>(w1 + 4 * i);
        x[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, o[i].x, x[0], 0, 0, 0);
        x[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, o[i].x, x[1], 0, 0, 0);
        x[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, o[i].y, x[0], 0, 0, 0);
        x[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, o[i].y, x[1], 0, 0, 0);
    }
}

// product 2: out[cb][r] += sum_w W[w][32 cb + mfma32_row(r, lg)] * x[w] over the 64 walked rows, for this lane's owned row
template <int D>
__device__ __forceinline__ void add_walked(const float* sW, const f32x16 (&x)[2], int li, int lg, f32x16 (&out)[mm_cb<D>()]) {
    constexpr int LD = mm_ld<D>(), CB = mm_cb<D>();
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* wrow = sW + (32 * b + mfma32_row(r, lg)) * LD + li;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                float a;
                if (32 * cb + 32 <= D) a = wrow[32 * cb];
                else a = 32 * cb + li < D ? wrow[32 * cb] : 0.f;        // the padded block: a register zero, nothing read
                out[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x[b][r], out[cb], 0, 0, 0);
            }
        }
}

// the owned row t of the result: channels 32 cb + 8 g + 4 lg .. + 3 from registers 4 g .. 4 g + 3, times mul
template <int D>
__device__ __forceinline__ void store_owned(const f32x16 (&out)[mm_cb<D>()], float* g, int cs, long row0, int t, int T, int lg, float mul) {
    if (t >= T) return;
    float* p = g + (row0 + t) * cs;
#pragma unroll
    for (int cb = 0; cb < mm_cb<D>(); ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (32 * cb + 8 * q + 8 > D) continue;                         // compile time: the padding of the last block
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = out[cb][4 * q + j] * mul;
            *reinterpret_cast<f32x4*>(p + 32 * cb + 8 * q + 4 * lg) = v;
        }
}

// logits of one tile in place: s * scale, -inf for walked keys >= Tk; returns their maximum over this lane's 32
__device__ __forceinline__ float scale_mask_max(f32x16 (&s)[2], int kt0, int Tk, int lg, float scale) {
    float mt = -INFINITY;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = kt0 + 32 * b + mfma32_row(r, lg) < Tk ? s[b][r] * scale : -INFINITY;
            s[b][r] = v;
            mt = fmaxf(mt, v);
        }
    return mt;
}

// ---------------------------------------------------------------------------------------------- forward
template <int D>
__global__ __launch_bounds__(256) void mha_mfma_fwd_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int Tq, int Tk, float scale) {
    constexpr int CB = mm_cb<D>();
    extern __shared__ float mm_lds[];
    float* sK = mm_lds;
    float* sV = sK + mm_tile_floats<D>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lg = lane >> 5;
    const int n = blockIdx.z, h = blockIdx.y, tq = blockIdx.x * MM_OWN + 32 * wave + li;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    float2 qr[D / 4];
    load_owned<D>(qr, qp, q.cs, (long)n * Tq, tq, Tq, lg);
    f32x16 o[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[cb][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int kt0 = 0; kt0 < Tk; kt0 += MM_TILE) {
        __syncthreads();                               // the previous tile's products have read sK and sV
        stage_tile<D>(sK, kp, k.cs, (long)n * Tk, kt0, Tk, tid);
        stage_tile<D>(sV, vp, v.cs, (long)n * Tk, kt0, Tk, tid);
        __syncthreads();
        f32x16 s[2];
        dot_head<D>(sK, qr, li, lg, s);
        float mt = scale_mask_max(s, kt0, Tk, lg, scale);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);          // finite: the tile holds at least one key, and the lane pair sees all 64
        const float alpha = expf(m_run - m_new);       // first tile: exp(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(s[b][r] - m_new);
                s[b][r] = p;
                ps += p;
            }
        ps += __shfl_xor(ps, 32, 64);                  // a + b on one lane, b + a on the other: the same bits
        l_run = l_run * alpha + ps;
        m_run = m_new;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) o[cb] *= alpha;
        add_walked<D>(sV, s, li, lg, o);
    }
    store_owned<D>(o, reinterpret_cast<float*>(y.p) + y.coff + h * D, y.cs, (long)n * Tq, tq, Tq, lg, 1.0f / l_run);
}

// ---------------------------------------------------------------------------------------------- backward
// mha_mfma_bwd_q_kernel owns queries: pass 1 walks the keys for (m, 1 / l, delta) per query, the running maximum and sum of the forward
// plus the running sum of p dP rescaled alike, into st[(n heads + h) Tq + i][3]; pass 2 (dq wanted) walks them again, dS in registers,
// dq += dS k.  mha_mfma_bwd_kv_kernel owns keys and walks the queries: P and dS in registers from the saved statistics (staged per
// tile as [64][4] in LDS: they vary along the registers there), dv += P dy, dk += dS q.  Query rows past Tq carry (0, 0, 0): P = 0.
template <int D>
__global__ __launch_bounds__(256) void mha_mfma_bwd_q_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, float* __restrict__ st,
                                                             int Tq, int Tk, float scale) {
    constexpr int CB = mm_cb<D>();
    extern __shared__ float mm_lds[];
    float* sK = mm_lds;
    float* sV = sK + mm_tile_floats<D>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lg = lane >> 5;
    const int n = blockIdx.z, h = blockIdx.y, heads = gridDim.y, tq = blockIdx.x * MM_OWN + 32 * wave + li;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    const float* __restrict__ gp = reinterpret_cast<const float*>(dy.p) + dy.coff + h * D;
    float2 qr[D / 4], gr[D / 4];
    load_owned<D>(qr, qp, q.cs, (long)n * Tq, tq, Tq, lg);
    load_owned<D>(gr, gp, dy.cs, (long)n * Tq, tq, Tq, lg);

    float m_run = -INFINITY, l_run = 0.f, d_run = 0.f;
    for (int kt0 = 0; kt0 < Tk; kt0 += MM_TILE) {
        __syncthreads();
        stage_tile<D>(sK, kp, k.cs, (long)n * Tk, kt0, Tk, tid);
        stage_tile<D>(sV, vp, v.cs, (long)n * Tk, kt0, Tk, tid);
        __syncthreads();
        f32x16 s[2], dp[2];
        dot_head<D>(sK, qr, li, lg, s);
        dot_head<D>(sV, gr, li, lg, dp);
        float mt = scale_mask_max(s, kt0, Tk, lg, scale);
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = expf(m_run - m_new);
        float ps = 0.f, pd = 0.f;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(s[b][r] - m_new);
                ps += p;
                pd = fmaf(p, dp[b][r], pd);
            }
        ps += __shfl_xor(ps, 32, 64);
        pd += __shfl_xor(pd, 32, 64);
        l_run = l_run * alpha + ps;
        d_run = d_run * alpha + pd;
        m_run = m_new;
    }
    const bool ok = tq < Tq;
    const float il = ok ? 1.0f / l_run : 0.f, dl = ok ? d_run * il : 0.f, mm = ok ? m_run : 0.f;
    if (ok && lg == 0) {
        float* o = st + (((long)n * heads + h) * Tq + tq) * 3;
        o[0] = mm;
        o[1] = il;
        o[2] = dl;
    }
    if (!dq.p) return;                                  // the whole block: uniform

    f32x16 o[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[cb][e] = 0.f;
    for (int kt0 = 0; kt0 < Tk; kt0 += MM_TILE) {
        __syncthreads();
        stage_tile<D>(sK, kp, k.cs, (long)n * Tk, kt0, Tk, tid);
        stage_tile<D>(sV, vp, v.cs, (long)n * Tk, kt0, Tk, tid);
        __syncthreads();
        f32x16 s[2], dp[2];
        dot_head<D>(sK, qr, li, lg, s);
        dot_head<D>(sV, gr, li, lg, dp);
        scale_mask_max(s, kt0, Tk, lg, scale);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) s[b][r] = expf(s[b][r] - mm) * il * (dp[b][r] - dl);
        add_walked<D>(sK, s, li, lg, o);
    }
    store_owned<D>(o, reinterpret_cast<float*>(dq.p) + dq.coff + h * D, dq.cs, (long)n * Tq, tq, Tq, lg, scale);
}

template <int D>
__global__ __launch_bounds__(256) void mha_mfma_bwd_kv_kernel(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dk, ssr_view dv,
                                                              const float* __restrict__ st, int Tq, int Tk, float scale) {
    constexpr int CB = mm_cb<D>();
    extern __shared__ float mm_lds[];
    float* sQ = mm_lds;
    float* sG = sQ + mm_tile_floats<D>();
    float* sSt = sG + mm_tile_floats<D>();             // [64][4]: m, 1 / l, delta, unused
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lg = lane >> 5;
    const int n = blockIdx.z, h = blockIdx.y, heads = gridDim.y, tk = blockIdx.x * MM_OWN + 32 * wave + li;
    const float* __restrict__ qp = reinterpret_cast<const float*>(q.p) + q.coff + h * D;
    const float* __restrict__ kp = reinterpret_cast<const float*>(k.p) + k.coff + h * D;
    const float* __restrict__ vp = reinterpret_cast<const float*>(v.p) + v.coff + h * D;
    const float* __restrict__ gp = reinterpret_cast<const float*>(dy.p) + dy.coff + h * D;
    float2 kr[D / 4], vr[D / 4];
    load_owned<D>(kr, kp, k.cs, (long)n * Tk, tk, Tk, lg);
    load_owned<D>(vr, vp, v.cs, (long)n * Tk, tk, Tk, lg);
    const bool key_ok = tk < Tk;
    f32x16 ok_[CB], ov_[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) ok_[cb][e] = ov_[cb][e] = 0.f;

    for (int qt0 = 0; qt0 < Tq; qt0 += MM_TILE) {
        __syncthreads();                               // the previous tile's products have read sQ, sG and sSt
        stage_tile<D>(sQ, qp, q.cs, (long)n * Tq, qt0, Tq, tid);
        stage_tile<D>(sG, gp, dy.cs, (long)n * Tq, qt0, Tq, tid);
        if (tid < MM_TILE) {
            const int t = qt0 + tid;
            f32x4 e = {0.f, 0.f, 0.f, 0.f};
            if (t < Tq) {
                const float* sp = st + (((long)n * heads + h) * Tq + t) * 3;
                e[0] = sp[0];
                e[1] = sp[1];
                e[2] = sp[2];
            }
            *reinterpret_cast<f32x4*>(sSt + 4 * tid) = e;
        }
        __syncthreads();
        f32x16 s[2], dp[2];
        dot_head<D>(sQ, kr, li, lg, s);
        dot_head<D>(sG, vr, li, lg, dp);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x4 e = *reinterpret_cast<const f32x4*>(sSt + 4 * (32 * b + mfma32_row(r, lg)));
                const float sv = key_ok ? s[b][r] * scale : -INFINITY;
                const float p = expf(sv - e[0]) * e[1];
                s[b][r] = p;
                dp[b][r] = p * (dp[b][r] - e[2]);
            }
        add_walked<D>(sG, s, li, lg, ov_);
        add_walked<D>(sQ, dp, li, lg, ok_);
    }
    store_owned<D>(ok_, reinterpret_cast<float*>(dk.p) + dk.coff + h * D, dk.cs, (long)n * Tk, tk, Tk, lg, scale);
    store_owned<D>(ov_, reinterpret_cast<float*>(dv.p) + dv.coff + h * D, dv.cs, (long)n * Tk, tk, Tk, lg, 1.0f);
}

template <int D> constexpr int mm_lds_bytes() { return (2 * mm_tile_floats<D>() + 4 * MM_TILE) * (int)sizeof(float); }

// 38 KB (head dim 72) or 34 KB (64) of LDS per workgroup: below the 64 KB that need no per-device opt-in (launch_mha of vit.hip needs one)
template <int D>
void launch_fwd(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int N, int Tq, int Tk, int heads, float scale, hipStream_t st) {
    constexpr int lds = mm_lds_bytes<D>();
    static_assert(lds <= 64 * 1024, "above 64 KB the kernels need hipFuncAttributeMaxDynamicSharedMemorySize, per device");
    hipLaunchKernelGGL(mha_mfma_fwd_kernel<D>, dim3((Tq + MM_OWN - 1) / MM_OWN, heads, N), dim3(256), lds, st, q, k, v, y, Tq, Tk, scale);
}

template <int D>
void launch_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws, int N, int Tq, int Tk,
                int heads, float scale, hipStream_t st) {
    constexpr int lds = mm_lds_bytes<D>();
    static_assert(lds <= 64 * 1024, "above 64 KB the kernels need hipFuncAttributeMaxDynamicSharedMemorySize, per device");
    hipLaunchKernelGGL(mha_mfma_bwd_q_kernel<D>, dim3((Tq + MM_OWN - 1) / MM_OWN, heads, N), dim3(256), lds, st, q, k, v, dy, dq, ws, Tq, Tk,
                       scale);
    hipLaunchKernelGGL(mha_mfma_bwd_kv_kernel<D>, dim3((Tk + MM_OWN - 1) / MM_OWN, heads, N), dim3(256), lds, st, q, k, v, dy, dk, dv, ws, Tq,
                       Tk, scale);
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define VIT_F32(dtype)                           \
    do {                                         \
        if (dtype == SSR_F32X3) dtype = SSR_F32; \
        if (dtype == SSR_BF16) return SSR_EUNSUP;\
        if (dtype != SSR_F32) return SSR_EINVAL; \
    } while (0)

extern "C" int ssr_mha_mfma_fwd(ssr_view q, ssr_view k, ssr_view v, ssr_view y, int32_t dtype, int32_t N, int32_t Tq, int32_t Tk,
                                int32_t heads, int32_t d, float scale, void* stream) {
    VIT_F32(dtype);
    if (N <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || !(scale == scale)) return SSR_EINVAL;
    if ((d != 64 && d != 72) || N > 65535 || heads > 65535 || Tq > (1 << 20) || Tk > (1 << 20)) return SSR_EUNSUP;
    const int C = heads * d;
    if (!view_ok(q, C) || !view_ok(k, C) || !view_ok(v, C) || !view_ok(y, C)) return SSR_EINVAL;
    const hipStream_t st = ST(stream);
    if (d == 64) launch_fwd<64>(q, k, v, y, N, Tq, Tk, heads, scale, st);
    else launch_fwd<72>(q, k, v, y, N, Tq, Tk, heads, scale, st);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int64_t ssr_mha_mfma_bwd_ws_floats(int32_t N, int32_t Tq, int32_t heads) {
    if (N <= 0 || Tq <= 0 || heads <= 0) return SSR_EINVAL;
    return 3 * (int64_t)N * heads * Tq;
}

extern "C" int ssr_mha_mfma_bwd(ssr_view q, ssr_view k, ssr_view v, ssr_view dy, ssr_view dq, ssr_view dk, ssr_view dv, float* ws,
                                int32_t dtype, int32_t N, int32_t Tq, int32_t Tk, int32_t heads, int32_t d, float scale, void* stream) {
    VIT_F32(dtype);
    if (N <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || !(scale == scale) || !ws || (reinterpret_cast<uintptr_t>(ws) & 3))
        return SSR_EINVAL;
    if ((d != 64 && d != 72) || N > 65535 || heads > 65535 || Tq > (1 << 20) || Tk > (1 << 20)) return SSR_EUNSUP;
    const int C = heads * d;
    if (!view_ok(q, C) || !view_ok(k, C) || !view_ok(v, C) || !view_ok(dy, C) || !view_ok(dk, C) || !view_ok(dv, C)) return SSR_EINVAL;
    if (dq.p && !view_ok(dq, C)) return SSR_EINVAL;
    const hipStream_t st = ST(stream);
    if (d == 64) launch_bwd<64>(q, k, v, dy, dq, dk, dv, ws, N, Tq, Tk, heads, scale, st);
    else launch_bwd<72>(q, k, v, dy, dq, dk, dv, ws, N, Tq, Tk, heads, scale, st);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
