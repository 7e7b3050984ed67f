// SelfAttentionBlock of the object-aware discriminator, forward and backward (include/ssr_hip.h, ssr_attn_desc).
//
// Replaces the device work of /root/reference/ssr/archs/osm_obj_discriminator_arch.py:16-31 (three 1x1 convolutions, two
// torch.bmm, softmax over the keys, gamma * out + x) and of autograd's backward of those lines.
//
// The shapes the network produces are tiny - (tokens N, channels C) = (64, 128) and (16, 256) for a 32 x 32 crop, ~4 MFLOP per
// image - so the block is bound by launches and latency, not by arithmetic.  One workgroup of 512 threads owns one image; every
// product is the same LDS micro-kernel: C[m][n] += sum_k A[k][m] * B[k][n] with both operands k-major in LDS, a 4 x 4 register
// tile per thread, one 16-byte read per operand and k.  Plain fp32 FMA (v_fma_f32): the fp32-input MFMA has the same peak rate
// as the vector unit on gfx950 and would add a fragment layout to every one of the eight products here.  The arithmetic is exact
// fp32 in every mode of the network.
//
// Forward : x -> xT (LDS), q / k / v projections with the weight matrices streamed from global memory in 16-row chunks
//           (transposed on the way into LDS; the next chunk is in flight in registers while the current one is consumed),
//           e = q k^T, max-subtracted softmax over the keys, out = a v, y = gamma * out + x.  a, q, k, v and out are SAVED for the
//           backward (<= 16 KB + 2 N C floats per image): the backward then needs no projection and no softmax.
// Backward: kernel 1, per image: dgamma partial, da = dy v^T, de (softmax backward), dq, dk, dv -> scratch [token][q | k | v],
//           dx = dy + [dq | dk | dv] W (weights streamed in their stored layout), optionally masked by relu'(x).
//           kernel 2, per 16 rows of [Wq; Wk; Wv]: dW += [dq | dk | dv]^T x and db += column sums over ALL tokens of ALL images in
//           token order, dgamma += the per-image partials in image order.  One writer per element, no atomics: two runs give the
//           same bytes.
#include "common.h"

namespace {

constexpr int AT_NT = 512;      // threads of an image workgroup
constexpr int AT_KC = 16;       // weight rows per streamed chunk
constexpr int AT_CC = 32;       // channels per chunk of da = dy v^T
constexpr int AT_WT = 256;      // threads of a parameter-gradient workgroup
constexpr int AT_WROWS = 16;    // rows of [Wq; Wk; Wv] per parameter-gradient workgroup
constexpr int AT_WTOK = 32;     // tokens per chunk there
constexpr int AT_MAX_LDS = 160 * 1024;

__host__ __device__ inline int at_max(int a, int b) { return a > b ? a : b; }

// per-image floats the forward saves: a [N][N], q [N][dk], k [N][dk], v [N][C], out [N][C]
__host__ __device__ inline int64_t at_save_floats(int N, int C) { return (int64_t)N * N + 2 * (int64_t)N * (C / 8) + 2 * (int64_t)N * C; }

struct FwdLds { int xT, att, aT, v, wt, qT, kT, total; };   // offsets in floats
__host__ __device__ inline FwdLds fwd_lds(int N, int C) {
    const int dk = C / 8, ldn = N + 4, ldc = C + 4;
    const int r1 = at_max(C * ldn, 2 * N * ldn);            // xT, later the energies and the transposed probabilities
    const int r2 = ldc * at_max(N, AT_KC);                  // weight chunk while projecting, then v
    FwdLds L;
    L.xT = 0; L.att = 0; L.aT = N * ldn;
    L.v = r1; L.wt = r1;
    L.qT = r1 + r2; L.kT = L.qT + dk * ldn;
    L.total = L.kT + dk * ldn;
    return L;
}

struct BwdLds { int de, an, deT, qn, kn, u, dyn, total; };
__host__ __device__ inline BwdLds bwd_lds(int N, int C) {
    const int dk = C / 8, ldn = N + 4, ldc = C + 4, ldd = dk + 4;
    BwdLds L;
    L.de = 0; L.an = N * ldn; L.deT = 2 * N * ldn;
    L.qn = 3 * N * ldn; L.kn = L.qn + N * ldd;
    L.u = L.kn + N * ldd;                                   // chunk buffers: (dy^T, v^T) of da, then (d^T, W) of dx
    L.dyn = L.u + at_max(2 * AT_CC * ldn, AT_KC * (ldn + ldc));
    L.total = L.dyn + N * ldc;
    return L;
}

// acc[4 r + s] += sum_k A[k * lda + r] * B[k * ldb + s]   (A, B 16-byte aligned LDS addresses)
__device__ __forceinline__ void mm4x4(float (&acc)[16], const float* A, int lda, const float* B, int ldb, int K) {
    for (int k = 0; k < K; ++k) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(A + k * lda);
        const f32x4 b = *reinterpret_cast<const f32x4*>(B + k * ldb);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[4 * r + s] = fmaf(a[r], b[s], acc[4 * r + s]);
    }
}

__device__ __forceinline__ f32x4 row_of(const float (&acc)[16], int r) { return f32x4{acc[4 * r], acc[4 * r + 1], acc[4 * r + 2], acc[4 * r + 3]}; }

// out[i][o] = b[o] + sum_k xT[k][i] W[o][k] for i < N, o < Cout (Cout % 4 == 0, Cout <= 256, C % AT_KC == 0).  W is streamed in chunks of
// AT_KC input channels, transposed into wt[k][o] (row stride Cout + 4).  emit(i0, o0, acc) receives every 4 x 4 tile once, after a barrier
// behind the last read of wt (the caller may overwrite it).
template <typename F>
__device__ __forceinline__ void project(const float* xT, int ldn, int N, int C, const float* __restrict__ W, const float* __restrict__ b,
                                        int Cout, float* wt, F emit) {
    const int tid = threadIdx.x, ldw = Cout + 4, tm = N >> 2, tiles = tm * (Cout >> 2), nvec = Cout * (AT_KC / 4);
    float acc[2][16];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = tid + u * AT_NT;
        const int o0 = t < tiles ? (t / tm) * 4 : 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float bv = b[o0 + s];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[u][4 * r + s] = bv;
        }
    }
    f32x4 pre[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + u * AT_NT;
            if (idx < nvec) pre[u] = *reinterpret_cast<const f32x4*>(W + (size_t)(idx >> 2) * C + k0 + 4 * (idx & 3));
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < C; k0 += AT_KC) {
        __syncthreads();                                    // the readers of the previous chunk are done
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + u * AT_NT;
            if (idx < nvec) {
#pragma unroll
                for (int e = 0; e < 4; ++e) wt[(4 * (idx & 3) + e) * ldw + (idx >> 2)] = pre[u][e];
            }
        }
        __syncthreads();
        if (k0 + AT_KC < C) fetch(k0 + AT_KC);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + u * AT_NT;
            if (t < tiles) mm4x4(acc[u], xT + k0 * ldn + (t % tm) * 4, ldn, wt + (t / tm) * 4, ldw, AT_KC);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int t = tid + u * AT_NT;
        if (t < tiles) emit((t % tm) * 4, (t / tm) * 4, acc[u]);
    }
}

__global__ __launch_bounds__(AT_NT) void attn_fwd_kernel(const ssr_attn_desc d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N = d.N, C = d.C, dk = C >> 3, ldn = N + 4, ldc = C + 4, tid = threadIdx.x, img = blockIdx.x, tm = N >> 2;
    const FwdLds L = fwd_lds(N, C);
    const float* __restrict__ xg = reinterpret_cast<const float*>(d.x.p) + (size_t)img * N * d.x.cs + d.x.coff;
    float* __restrict__ yg = reinterpret_cast<float*>(d.y.p) + (size_t)img * N * d.y.cs + d.y.coff;
    float* sv = d.save ? d.save + (size_t)img * at_save_floats(N, C) : nullptr;
    float* sA = sv;
    float* sq = sv ? sv + N * N : nullptr;
    float* sk = sv ? sq + N * dk : nullptr;
    float* svv = sv ? sk + N * dk : nullptr;
    float* so = sv ? svv + N * C : nullptr;

    // x -> xT[c][i]  (token i = h * W + w: the pixel order of the NHWC buffer, osm_obj_discriminator_arch.py:20)
    for (int idx = tid; idx < N * (C >> 2); idx += AT_NT) {
        const int i = idx % N, c4 = idx / N;
        const f32x4 v = *reinterpret_cast<const f32x4*>(xg + (size_t)i * d.x.cs + 4 * c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[L.xT + (4 * c4 + e) * ldn + i] = v[e];
    }
    float* qT = lds + L.qT;
    float* kT = lds + L.kT;
    float* vn = lds + L.v;
    project(lds + L.xT, ldn, N, C, d.wq, d.bq, dk, lds + L.wt, [&](int i0, int o0, const float (&acc)[16]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < 4; ++s) qT[(o0 + s) * ldn + i0 + r] = acc[4 * r + s];
            if (sv) *reinterpret_cast<f32x4*>(sq + (i0 + r) * dk + o0) = row_of(acc, r);
        }
    });
    project(lds + L.xT, ldn, N, C, d.wk, d.bk, dk, lds + L.wt, [&](int i0, int o0, const float (&acc)[16]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int s = 0; s < 4; ++s) kT[(o0 + s) * ldn + i0 + r] = acc[4 * r + s];
            if (sv) *reinterpret_cast<f32x4*>(sk + (i0 + r) * dk + o0) = row_of(acc, r);
        }
    });
    project(lds + L.xT, ldn, N, C, d.wv, d.bv, C, lds + L.wt, [&](int i0, int o0, const float (&acc)[16]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<f32x4*>(vn + (i0 + r) * ldc + o0) = row_of(acc, r);
            if (sv) *reinterpret_cast<f32x4*>(svv + (i0 + r) * C + o0) = row_of(acc, r);
        }
    });
    __syncthreads();
    // e[i][j] = q_i . k_j  (xT is dead: its region takes the energies)
    float* att = lds + L.att;
    float* aT = lds + L.aT;
    for (int t = tid; t < tm * tm; t += AT_NT) {
        const int i0 = (t % tm) * 4, j0 = (t / tm) * 4;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        mm4x4(acc, qT + i0, ldn, kT + j0, ldn, dk);
#pragma unroll
        for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(att + (i0 + r) * ldn + j0) = row_of(acc, r);
    }
    __syncthreads();
    // softmax over the keys, eight lanes per query row: exp(e - max) / sum  (torch.softmax(energy, dim=2), :24)
    {
        const int row = tid >> 3, l = tid & 7;
        const bool valid = row < N;
        float m = -INFINITY;
        float p[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = l + 8 * q;
            p[q] = (valid && j < N) ? att[row * ldn + j] : -INFINITY;
            m = fmaxf(m, p[q]);
        }
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        m = fmaxf(m, __shfl_xor(m, 4));
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = l + 8 * q;
            p[q] = (valid && j < N) ? expf(p[q] - m) : 0.f;
            s += p[q];
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = l + 8 * q;
            if (valid && j < N) {
                const float a = p[q] / s;
                aT[j * ldn + row] = a;
                if (sv) sA[row * N + j] = a;
            }
        }
    }
    __syncthreads();
    // out_i = sum_j a[i][j] v_j ;  y = gamma * out + x   (:27-30)
    const float g = d.gamma[0];
    for (int t = tid; t < tm * (C >> 2); t += AT_NT) {
        const int i0 = (t % tm) * 4, c0 = (t / tm) * 4;
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        mm4x4(acc, aT + i0, ldn, vn + c0, ldc, N);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 o = row_of(acc, r);
            if (sv) *reinterpret_cast<f32x4*>(so + (i0 + r) * C + c0) = o;
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xg + (size_t)(i0 + r) * d.x.cs + c0);
            f32x4 yv;
#pragma unroll
            for (int e = 0; e < 4; ++e) yv[e] = fmaf(g, o[e], xv[e]);
            *reinterpret_cast<f32x4*>(yg + (size_t)(i0 + r) * d.y.cs + c0) = yv;
        }
    }
}

// backward, kernel 1: one image per workgroup
__global__ __launch_bounds__(AT_NT) void attn_bwd_kernel(const ssr_attn_desc d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N = d.N, C = d.C, dk = C >> 3, ldn = N + 4, ldc = C + 4, ldd = dk + 4, tid = threadIdx.x, img = blockIdx.x, tm = N >> 2;
    const int Ct = C + 2 * dk;
    const BwdLds L = bwd_lds(N, C);
    const float* __restrict__ dyg = reinterpret_cast<const float*>(d.dy.p) + (size_t)img * N * d.dy.cs + d.dy.coff;
    const float* __restrict__ xg = reinterpret_cast<const float*>(d.x.p) + (size_t)img * N * d.x.cs + d.x.coff;
    float* __restrict__ dxg = reinterpret_cast<float*>(d.dx.p) + (size_t)img * N * d.dx.cs + d.dx.coff;
    const float* sv = d.save + (size_t)img * at_save_floats(N, C);
    const float* sA = sv;
    const float* sq = sv + N * N;
    const float* sk = sq + N * dk;
    const float* svv = sk + N * dk;
    const float* so = svv + N * C;
    float* dqkv = d.scratch + (size_t)img * N * Ct;            // [token][dq | dk | dv]
    float* gpart = d.scratch + (size_t)d.Bo * N * Ct;          // per-image partial of dgamma
    float* de = lds + L.de;
    float* an = lds + L.an;
    float* deT = lds + L.deT;
    float* qn = lds + L.qn;
    float* kn = lds + L.kn;
    float* dyn = lds + L.dyn;
    float* ub = lds + L.u;
    const float g = d.gamma[0];

    // dy, a, q, k into LDS as stored; dgamma partial = sum dy * out, summed in a fixed order
    float gs = 0.f;
    for (int idx = tid; idx < N * (C >> 2); idx += AT_NT) {
        const int i = idx / (C >> 2), c4 = idx % (C >> 2);
        const f32x4 v = *reinterpret_cast<const f32x4*>(dyg + (size_t)i * d.dy.cs + 4 * c4);
        const f32x4 o = *reinterpret_cast<const f32x4*>(so + i * C + 4 * c4);
        *reinterpret_cast<f32x4*>(dyn + i * ldc + 4 * c4) = v;
#pragma unroll
        for (int e = 0; e < 4; ++e) gs = fmaf(v[e], o[e], gs);
    }
    for (int idx = tid; idx < N * (N >> 2); idx += AT_NT) {
        const int i = idx / (N >> 2), j4 = idx % (N >> 2);
        *reinterpret_cast<f32x4*>(an + i * ldn + 4 * j4) = *reinterpret_cast<const f32x4*>(sA + i * N + 4 * j4);
    }
    for (int idx = tid; idx < N * (dk >> 2); idx += AT_NT) {
        const int i = idx / (dk >> 2), d4 = idx % (dk >> 2);
        *reinterpret_cast<f32x4*>(qn + i * ldd + 4 * d4) = *reinterpret_cast<const f32x4*>(sq + i * dk + 4 * d4);
        *reinterpret_cast<f32x4*>(kn + i * ldd + 4 * d4) = *reinterpret_cast<const f32x4*>(sk + i * dk + 4 * d4);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) gs += __shfl_xor(gs, m);
    if ((tid & 63) == 0) ub[tid >> 6] = gs;
    __syncthreads();
    if (tid == 0) {
        float s = 0.f;
        for (int w = 0; w < AT_NT / 64; ++w) s += ub[w];
        gpart[img] = s;
    }
    // da[i][j] = sum_c dy[i][c] v[j][c], channels in chunks of AT_CC (both operands transposed into the chunk buffers)
    {
        float acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float* dyT = ub;
        float* vT = ub + AT_CC * ldn;
        const int i0 = (tid % tm) * 4, j0 = (tid / tm) * 4;
        for (int c0 = 0; c0 < C; c0 += AT_CC) {
            __syncthreads();
            for (int idx = tid; idx < N * (AT_CC / 4); idx += AT_NT) {
                const int i = idx % N, c4 = idx / N;
                const f32x4 a = *reinterpret_cast<const f32x4*>(dyn + i * ldc + c0 + 4 * c4);
                const f32x4 b = *reinterpret_cast<const f32x4*>(svv + i * C + c0 + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dyT[(4 * c4 + e) * ldn + i] = a[e];
                    vT[(4 * c4 + e) * ldn + i] = b[e];
                }
            }
            __syncthreads();
            if (tid < tm * tm) mm4x4(acc, dyT + i0, ldn, vT + j0, ldn, AT_CC);
        }
        if (tid < tm * tm) {
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(de + (i0 + r) * ldn + j0) = row_of(acc, r);
        }
    }
    __syncthreads();
    // softmax backward, eight lanes per row: de = gamma * a * (da - sum_j a da)
    {
        const int row = tid >> 3, l = tid & 7;
        const bool valid = row < N;
        float a[8], da[8], rs = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = l + 8 * q;
            const bool ok = valid && j < N;
            a[q] = ok ? an[row * ldn + j] : 0.f;
            da[q] = ok ? de[row * ldn + j] : 0.f;
            rs = fmaf(a[q], da[q], rs);
        }
        rs += __shfl_xor(rs, 1);
        rs += __shfl_xor(rs, 2);
        rs += __shfl_xor(rs, 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int j = l + 8 * q;
            if (valid && j < N) {
                const float v = g * (a[q] * (da[q] - rs));
                de[row * ldn + j] = v;
                deT[j * ldn + row] = v;
            }
        }
    }
    __syncthreads();
    // dq_i = sum_j de[i][j] k_j ;  dk_j = sum_i de[i][j] q_i ;  dv_j = gamma * sum_i a[i][j] dy_i   -> scratch
    {
        const int tq = tm * (dk >> 2);
        for (int t = tid; t < 2 * tq; t += AT_NT) {
            const bool second = t >= tq;
            const int tt = second ? t - tq : t;
            const int i0 = (tt % tm) * 4, d0 = (tt / tm) * 4;
            float acc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            mm4x4(acc, (second ? de : deT) + i0, ldn, (second ? qn : kn) + d0, ldd, N);
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(dqkv + (size_t)(i0 + r) * Ct + (second ? dk : 0) + d0) = row_of(acc, r);
        }
        for (int t = tid; t < tm * (C >> 2); t += AT_NT) {
            const int j0 = (t % tm) * 4, c0 = (t / tm) * 4;
            float acc[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            mm4x4(acc, an + j0, ldn, dyn + c0, ldc, N);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f32x4 v = row_of(acc, r);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= g;
                *reinterpret_cast<f32x4*>(dqkv + (size_t)(j0 + r) * Ct + 2 * dk + c0) = v;
            }
        }
    }
    __syncthreads();                                        // this workgroup's scratch rows are visible to all of its threads
    // dx[i][c] = dy[i][c] + sum_o [dq | dk | dv][i][o] * [Wq; Wk; Wv][o][c], rows o streamed in chunks of AT_KC
    {
        float* dT = ub;                                     // [AT_KC][ldn]
        float* wc = ub + AT_KC * ldn;                       // [AT_KC][ldc]
        const int tiles = tm * (C >> 2), nw = AT_KC * (C >> 2), nd = N * (AT_KC / 4);
        float acc[2][16];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
        f32x4 prew[2], pred;
        auto fetch = [&](int o0) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = tid + u * AT_NT;
                if (idx < nw) {
                    const int o = o0 + idx / (C >> 2), c4 = idx % (C >> 2);
                    const float* row = o < dk ? d.wq + (size_t)o * C : o < 2 * dk ? d.wk + (size_t)(o - dk) * C : d.wv + (size_t)(o - 2 * dk) * C;
                    prew[u] = o < Ct ? *reinterpret_cast<const f32x4*>(row + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (tid < nd) {
                const int i = tid % N, o = o0 + 4 * (tid / N);
                pred = o < Ct ? *reinterpret_cast<const f32x4*>(dqkv + (size_t)i * Ct + o) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        };
        fetch(0);
        for (int o0 = 0; o0 < Ct; o0 += AT_KC) {
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int idx = tid + u * AT_NT;
                if (idx < nw) *reinterpret_cast<f32x4*>(wc + (idx / (C >> 2)) * ldc + 4 * (idx % (C >> 2))) = prew[u];
            }
            if (tid < nd) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dT[(4 * (tid / N) + e) * ldn + tid % N] = pred[e];
            }
            __syncthreads();
            if (o0 + AT_KC < Ct) fetch(o0 + AT_KC);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = tid + u * AT_NT;
                if (t < tiles) mm4x4(acc[u], dT + (t % tm) * 4, ldn, wc + (t / tm) * 4, ldc, AT_KC);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = tid + u * AT_NT;
            if (t < tiles) {
                const int i0 = (t % tm) * 4, c0 = (t / tm) * 4;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const f32x4 dyv = *reinterpret_cast<const f32x4*>(dyn + (i0 + r) * ldc + c0);
                    f32x4 v = row_of(acc[u], r);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += dyv[e];
                    if (d.relu_mask) {
                        const f32x4 xv = *reinterpret_cast<const f32x4*>(xg + (size_t)(i0 + r) * d.x.cs + c0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = xv[e] > 0.f ? v[e] : 0.f;
                    }
                    *reinterpret_cast<f32x4*>(dxg + (size_t)(i0 + r) * d.dx.cs + c0) = v;
                }
            }
        }
    }
}

// backward, kernel 2: AT_WROWS rows of [Wq; Wk; Wv] per workgroup, every token of every image in order
__global__ __launch_bounds__(AT_WT) void attn_wgrad_kernel(const ssr_attn_desc d) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int N = d.N, C = d.C, dk = C >> 3, ldc = C + 4, tid = threadIdx.x, Ct = C + 2 * dk;
    constexpr int LDD = AT_WROWS + 4;
    const int T = d.Bo * N, o0 = blockIdx.x * AT_WROWS;
    float* dch = lds;                                       // [AT_WTOK][LDD]
    float* xch = lds + AT_WTOK * LDD;                       // [AT_WTOK][ldc]
    const float* __restrict__ xg = reinterpret_cast<const float*>(d.x.p) + d.x.coff;
    const float* __restrict__ dqkv = d.scratch;
    const bool active = tid < C;                            // 4 row groups x C / 4 column groups
    const int orow = (tid & 3) * 4, c0 = (tid >> 2) * 4;
    const int nx = AT_WTOK * (C >> 2);
    float acc[16], bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 prex[8], pred;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int t0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + u * AT_WT;
            if (idx < nx) {
                const int tok = t0 + idx / (C >> 2), c4 = idx % (C >> 2);
                prex[u] = tok < T ? *reinterpret_cast<const f32x4*>(xg + (size_t)tok * d.x.cs + 4 * c4) : zero;
            }
        }
        if (tid < AT_WTOK * (AT_WROWS / 4)) {
            const int tok = t0 + tid / (AT_WROWS / 4), o = o0 + 4 * (tid % (AT_WROWS / 4));
            pred = (tok < T && o < Ct) ? *reinterpret_cast<const f32x4*>(dqkv + (size_t)tok * Ct + o) : zero;
        }
    };
    fetch(0);
    for (int t0 = 0; t0 < T; t0 += AT_WTOK) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = tid + u * AT_WT;
            if (idx < nx) *reinterpret_cast<f32x4*>(xch + (idx / (C >> 2)) * ldc + 4 * (idx % (C >> 2))) = prex[u];
        }
        if (tid < AT_WTOK * (AT_WROWS / 4)) *reinterpret_cast<f32x4*>(dch + (tid / (AT_WROWS / 4)) * LDD + 4 * (tid % (AT_WROWS / 4))) = pred;
        __syncthreads();
        if (t0 + AT_WTOK < T) fetch(t0 + AT_WTOK);
        if (active) {
            mm4x4(acc, dch + orow, LDD, xch + c0, ldc, AT_WTOK);
            if (c0 == 0) {
                for (int k = 0; k < AT_WTOK; ++k) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(dch + k * LDD + orow);
#pragma unroll
                    for (int r = 0; r < 4; ++r) bsum[r] += a[r];
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = o0 + orow + r;
            if (o >= Ct) continue;
            float* dw = o < dk ? d.dwq + (size_t)o * C : o < 2 * dk ? d.dwk + (size_t)(o - dk) * C : d.dwv + (size_t)(o - 2 * dk) * C;
            float* db = o < dk ? d.dbq + o : o < 2 * dk ? d.dbk + (o - dk) : d.dbv + (o - 2 * dk);
            f32x4 v = *reinterpret_cast<const f32x4*>(dw + c0);
            const f32x4 a = row_of(acc, r);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += a[e];
            *reinterpret_cast<f32x4*>(dw + c0) = v;
            if (c0 == 0) *db += bsum[r];
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        const float* gpart = d.scratch + (size_t)T * Ct;
        float s = 0.f;
        for (int b = 0; b < d.Bo; ++b) s += gpart[b];
        d.dgamma[0] += s;
    }
}

// dst = g where y > 0, else 0, over C channels of npix pixels
__global__ __launch_bounds__(256) void relu_bwd_kernel(ssr_view g, ssr_view y, ssr_view dst, int64_t npix, int C) {
    const int64_t n = npix * C;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t p = e / C;
        const int c = (int)(e - p * C);
        const float yv = reinterpret_cast<const float*>(y.p)[p * y.cs + y.coff + c];
        const float gv = reinterpret_cast<const float*>(g.p)[p * g.cs + g.coff + c];
        reinterpret_cast<float*>(dst.p)[p * dst.cs + dst.coff + c] = yv > 0.f ? gv : 0.f;
    }
}

bool al16(const void* p) { return p && ((uintptr_t)p % 16) == 0; }
bool al4(const void* p) { return p && ((uintptr_t)p % 4) == 0; }
bool attn_view_ok(const ssr_view& v, int C) { return al16(v.p) && v.cs > 0 && (v.cs % 4) == 0 && v.coff >= 0 && (v.coff % 4) == 0 && v.coff + C <= v.cs; }

// SSR_OK, or the code the entry returns without a launch
int attn_check(const ssr_attn_desc* d, bool bwd) {
    if (!d || d->Bo <= 0 || d->C <= 0 || (d->C % 8) != 0) return SSR_EINVAL;
    if (!(d->N == 4 || d->N == 8 || d->N == 16 || d->N == 32 || d->N == 64)) return SSR_EINVAL;
    if (!attn_view_ok(d->x, d->C)) return SSR_EINVAL;
    if (!al16(d->wq) || !al16(d->wk) || !al16(d->wv) || !al4(d->gamma)) return SSR_EINVAL;
    if (!bwd) {
        if (!attn_view_ok(d->y, d->C) || !al4(d->bq) || !al4(d->bk) || !al4(d->bv) || (d->save && !al16(d->save))) return SSR_EINVAL;
    } else {
        if (!attn_view_ok(d->dy, d->C) || !attn_view_ok(d->dx, d->C) || !al16(d->save) || !al16(d->scratch)) return SSR_EINVAL;
        const int ng = (d->dwq != nullptr) + (d->dbq != nullptr) + (d->dwk != nullptr) + (d->dbk != nullptr) + (d->dwv != nullptr) +
                       (d->dbv != nullptr) + (d->dgamma != nullptr);
        if (ng != 0 && ng != 7) return SSR_EINVAL;          // all parameter gradients, or none (a frozen discriminator)
        if (ng && (!al16(d->dwq) || !al16(d->dwk) || !al16(d->dwv) || !al4(d->dbq) || !al4(d->dbk) || !al4(d->dbv) || !al4(d->dgamma)))
            return SSR_EINVAL;
    }
    if ((d->C % 32) != 0 || d->C > 256) return SSR_EUNSUP;
    if ((int64_t)d->Bo * d->N * (d->C + d->C / 4) > 0x7fffff00LL / 4) return SSR_EUNSUP;
    return SSR_OK;
}

template <typename K>
int attn_lds_optin(K kern, bool (&done)[SSR_MAX_DEVICES]) {
    const int dev = ssr_device_ordinal();
    if (!done[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, AT_MAX_LDS);
        if (e != hipSuccess) return (int)e;
        done[dev] = true;
    }
    return SSR_OK;
}

}  // namespace

extern "C" int64_t ssr_self_attention_save_floats(int32_t N, int32_t C) {
    if (N <= 0 || C <= 0 || (C % 8) != 0) return 0;
    return at_save_floats(N, C);
}

extern "C" int64_t ssr_self_attention_scratch_floats(int32_t Bo, int32_t N, int32_t C) {
    if (Bo <= 0 || N <= 0 || C <= 0 || (C % 8) != 0) return 0;
    return (((int64_t)Bo * N * (C + C / 4) + Bo) + 3) / 4 * 4;
}

extern "C" int ssr_self_attention_fwd(const ssr_attn_desc* d, void* stream) {
    const int rc = attn_check(d, false);
    if (rc != SSR_OK) return rc;
    const size_t lds = (size_t)fwd_lds(d->N, d->C).total * sizeof(float);
    if (lds > (size_t)AT_MAX_LDS) return SSR_EUNSUP;
    static bool done[SSR_MAX_DEVICES] = {};
    const int rca = attn_lds_optin(attn_fwd_kernel, done);
    if (rca != SSR_OK) return rca;
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(d->Bo), dim3(AT_NT), lds, reinterpret_cast<hipStream_t>(stream), *d);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_self_attention_bwd(const ssr_attn_desc* d, void* stream) {
    const int rc = attn_check(d, true);
    if (rc != SSR_OK) return rc;
    const size_t lds = (size_t)bwd_lds(d->N, d->C).total * sizeof(float);
    if (lds > (size_t)AT_MAX_LDS) return SSR_EUNSUP;
    static bool done[SSR_MAX_DEVICES] = {};
    const int rca = attn_lds_optin(attn_bwd_kernel, done);
    if (rca != SSR_OK) return rca;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(attn_bwd_kernel, dim3(d->Bo), dim3(AT_NT), lds, st, *d);
    SSR_LAUNCH_CHECK();
    if (d->dwq) {
        const int Ct = d->C + d->C / 4;
        const size_t ldw = (size_t)(AT_WTOK * (AT_WROWS + 4) + AT_WTOK * (d->C + 4)) * sizeof(float);
        hipLaunchKernelGGL(attn_wgrad_kernel, dim3((Ct + AT_WROWS - 1) / AT_WROWS), dim3(AT_WT), ldw, st, *d);
        SSR_LAUNCH_CHECK();
    }
    return SSR_OK;
}

extern "C" int ssr_relu_bwd(ssr_view g, ssr_view y, ssr_view dst, int64_t npix, int32_t C, void* stream) {
    auto ok = [&](const ssr_view& v) { return al4(v.p) && v.cs > 0 && v.coff >= 0 && v.coff + C <= v.cs; };
    if (npix <= 0 || C <= 0 || !ok(g) || !ok(y) || !ok(dst)) return SSR_EINVAL;
    const int64_t n = npix * C;
    const int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, y, dst, npix, (int)C);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
