// Scene inference glue: a whole Sentinel-2 image stack stays on the device between its upload and the download of the
// super-resolved mosaic (satlas_super_resolution_amd/infer_scene.py).  Byte work around the generator, HBM-bound, a few tens of MB
// per 512 x 512 tile next to 9.4 TFLOP of convolutions.
//
//   ssr_scene_zero_scan    per (chunk, frame): does the 32 x 32 x 3 block hold a zero sample (`[0, 0, 0] in ts`,
//                          ssr/utils/infer_utils.py:17 of the reference)
//   ssr_scene_gather       the chosen frames of a batch of chunks -> the generator plan's NHWC input, / 255 (infer_utils.py:33-38)
//   ssr_scene_scatter_u8   the plan's NHWC output -> truncating uint8 (infer_grid.py:60-64) at the chunks' places in the mosaic
//                          (infer_utils.py:41-60), counting non-finite samples
//
// A scene is uint8 [T][H][W][3], H and W multiples of 32: a chunk row is 96 contiguous bytes (6 x 16) and a row of a
// super-resolved chunk 128 * C bytes of the mosaic, both 16-byte aligned when the base pointers are - the global accesses on the
// byte side are uint4.  Chunk and frame ids come from device arrays; an id outside the scene makes its item a no-op (nothing is
// read or written for it).
//
// Overlap-and-blend for scenes of ANY size >= 32 x 32 (super_resolve_scene_blended): chunks sit at arbitrary (y0, x0), given as a
// device array of int32 pairs, overlap, and are cross-faded in the output in integer arithmetic.
//
//   ssr_scene_zero_scan_at   the zero test over the 32 x 32 windows at the origins
//   ssr_scene_gather_at      ssr_scene_gather at the origins
//   ssr_scene_blend_add      the plan's NHWC output -> 16-bit fixed point, times the window weight of its place in the chunk,
//                            added (integer atomics: any arrival order gives the same words) into a uint32 accumulator
//   ssr_scene_blend_finish   accumulator / weight sums -> the truncating uint8 mosaic
//
// Multi-band generators (`s2_bands: [tci, b05, ...]`): K extra bands lie beside the TCI as uint8 [K][T][H][W], one plane per band.
//
//   ssr_scene_gather_bands   ssr_scene_gather_at with 3 + K channels per chosen frame: the TCI pixel, then the K band samples
//
// Frame choice on the device (`frame_select: clearest`, this project's own policy: the reference has no counterpart file): per
// (chunk, frame) a key that counts the window's NODATA and saturated pixels, per chunk the n frames of the smallest (key, index).
//
//   ssr_scene_frame_keys     per (chunk at an origin, frame): (pixels with a zero sample << 16) | pixels that are (255, 255, 255)
//   ssr_scene_rank_frames    per chunk: its T keys ranked by (key, frame index), the first n frame indices -> frame_ids
//
// NODATA in, NODATA out (`nodata: keep`, this project's own policy: the reference has no counterpart file): a low-resolution pixel of
// a frame HAS DATA if none of its three TCI samples is 0 (the complement of ssr_scene_frame_keys' z); support[y][x] counts the
// (covering chunk, chosen frame slot) pairs whose pixel has data - exactly what went into the generator.
//
//   ssr_scene_support_add    per chunk at an origin: the slots whose frame has data, per pixel of the window, added (integer
//                            atomics) to an int32 [H][W] support map
//   ssr_scene_apply_nodata   the uint8 mosaic in place: the 4 x 4 block of a pixel with support < min_support becomes 0, every other
//                            sample max(1, sample) (0 stays reserved for NODATA); min(support, 255) as a uint8 [H][W] map
//
// Self-ensemble (`self_ensemble: true`: BasicSR's val.self_ensemble transform set, averaged by the integer blend): a generator row
// is a (chunk, transform) pair, the transform id tf in 0 .. 7 with bit 0 = flip the columns, bit 1 = flip the rows, bit 2 =
// transpose, applied in that order.
//
//   ssr_scene_gather_tf            ssr_scene_gather_at / ssr_scene_gather_bands, the chunk written under its row's transform
//   ssr_scene_blend_add_tf         ssr_scene_blend_add of the output turned back, in 13-bit fixed point (eight rows per chunk fit)
//   ssr_scene_blend_finish_scaled  ssr_scene_blend_finish with the denominator's scale (8 * 8191) as an argument
//
// Here a chunk row of the scene starts at any byte (W * 3 may be odd) and a mosaic row is only 4-byte aligned: rows are read as the
// aligned words that lie inside them plus single bytes at the two ends, the mosaic is stored in aligned 4-byte units.
#include "common.h"

namespace {

constexpr int CH = 32;             // low-resolution chunk edge
constexpr int ROW16 = CH * 3 / 16; // uint4 per chunk row of the scene
constexpr int SR = 128;            // super-resolved chunk edge (scale 4)
constexpr int SROWS = 8;           // mosaic rows per scatter block
constexpr int MAX_C = 8;           // output channels ssr_scene_scatter_u8 accepts
constexpr float INV255 = 1.0f / 255.0f;

__device__ __forceinline__ bool has_zero_byte(uint32_t v) { return ((v - 0x01010101u) & ~v & 0x80808080u) != 0; }

// one wave per (chunk, frame): 192 uint4 = 3 per lane
__global__ __launch_bounds__(256) void scene_zero_scan_kernel(const uint8_t* __restrict__ scene, int T, int H, int W,
                                                              uint8_t* __restrict__ has_zero) {
    const int gw = W / CH, n_chunks = (H / CH) * gw;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)n_chunks * T) return;                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int chunk = (int)(item / T), t = (int)(item - (long)chunk * T);
    const int ci = chunk / gw, cj = chunk - ci * gw;
    const uint8_t* base = scene + (((long)t * H + (long)ci * CH) * W + (long)cj * CH) * 3;
    bool z = false;
#pragma unroll
    for (int k = 0; k < CH * ROW16 / 64; ++k) {
        const int e = lane + 64 * k, row = e / ROW16, q = e - row * ROW16;
        const uint4 v = *reinterpret_cast<const uint4*>(base + (long)row * W * 3 + 16 * q);
        z |= has_zero_byte(v.x) | has_zero_byte(v.y) | has_zero_byte(v.z) | has_zero_byte(v.w);
    }
    const bool any = __any(z);
    if (lane == 0) has_zero[item] = any ? 1 : 0;
}

template <typename T, int V> struct Pack;
template <typename T> struct Pack<T, 1> { T v[1]; };
template <> struct alignas(16) Pack<float, 4> { float v[4]; };
template <> struct alignas(16) Pack<__bf16, 8> { __bf16 v[8]; };

// one block per (batch item, chunk row): the n chosen frames' rows go through LDS (n * 96 bytes), then V consecutive channels of a
// pixel per thread and store (V = 16 bytes when 3 n is a multiple of it, else single elements).  Consecutive threads write
// consecutive addresses inside a pixel and on to the next one (contiguous when the view has no pad).
template <typename T, int V>
__global__ __launch_bounds__(256) void scene_gather_kernel(const uint8_t* __restrict__ scene, int T_, int H, int W,
                                                           const int32_t* __restrict__ chunk_ids,
                                                           const int32_t* __restrict__ frame_ids, int n, ssr_view dst) {
    extern __shared__ uint4 rows[];                               // [n][ROW16]
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    const int gw = W / CH, chunk = chunk_ids[b];
    if (chunk < 0 || chunk >= (H / CH) * gw) return;              // block-uniform
    const int ci = chunk / gw, cj = chunk - ci * gw;
    for (int k = 0; k < n; ++k) {                                 // block-uniform: before any barrier
        const int f = frame_ids[b * n + k];
        if (f < 0 || f >= T_) return;
    }
    for (int e = threadIdx.x; e < n * ROW16; e += 256) {
        const int k = e / ROW16, q = e - k * ROW16;
        const long t = frame_ids[b * n + k];
        rows[e] = *reinterpret_cast<const uint4*>(scene + ((t * H + (long)ci * CH + y) * W + (long)cj * CH) * 3 + 16 * q);
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(rows);
    const int C = 3 * n, groups = C / V;
    T* __restrict__ d = reinterpret_cast<T*>(dst.p);
    const long pix0 = ((long)b * CH + y) * CH;
    for (int e = threadIdx.x; e < CH * groups; e += 256) {
        const int x = e / groups, c0 = (e - x * groups) * V;
        Pack<T, V> o;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int c = c0 + u, k = c / 3;
            // `.float() / 255` of frames_to_input ON THE DEVICE: ATen's division of a tensor by a host scalar multiplies by the
            // reciprocal rounded to fp32 (x * (1.0f / 255.0f); 126 of the 256 byte values differ from x / 255.0f in the last bit),
            // then the storage type's rounding (ssr_nchw_to_nhwc)
            o.v[u] = from_f32<T>((float)bytes[k * (CH * 3) + x * 3 + (c - 3 * k)] * INV255);
        }
        *reinterpret_cast<Pack<T, V>*>(d + (pix0 + x) * dst.cs + dst.coff + c0) = o;
    }
}

template <typename T> __device__ __forceinline__ void load_pixel(const T* p, int C, float (&v)[MAX_C]);
template <> __device__ __forceinline__ void load_pixel<float>(const float* p, int C, float (&v)[MAX_C]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);          // a pixel of the view starts on 32 bytes (cs, coff % 8 == 0)
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = a[u];
    if (C > 4) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[4 + u] = b[u];
    }
}
template <> __device__ __forceinline__ void load_pixel<__bf16>(const __bf16* p, int C, float (&v)[MAX_C]) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (float)a[u];
}

// one block per (batch item, SROWS rows of its 128 x 128 output): pixels are read whole (the first 8 channels of the view in one
// or two 16-byte loads), quantised into an LDS image of the rows, and leave as uint4 stores into the mosaic
template <typename T>
__global__ __launch_bounds__(256) void scene_scatter_u8_kernel(ssr_view src, const int32_t* __restrict__ chunk_ids, int C,
                                                               uint8_t* __restrict__ mosaic, int Ho, int Wo,
                                                               int32_t* __restrict__ nonfinite) {
    __shared__ uint4 img[SROWS * SR * MAX_C / 16];
    uint8_t* bytes = reinterpret_cast<uint8_t*>(img);
    const int b = blockIdx.x / (SR / SROWS), y0 = (blockIdx.x - b * (SR / SROWS)) * SROWS;
    const int gw = Wo / SR, chunk = chunk_ids[b];
    if (chunk < 0 || chunk >= (Ho / SR) * gw) return;             // block-uniform
    const int ci = chunk / gw, cj = chunk - ci * gw;
    const T* __restrict__ s = reinterpret_cast<const T*>(src.p);
    int bad = 0;
#pragma unroll
    for (int it = 0; it < SROWS * SR / 256; ++it) {
        const int e = threadIdx.x + 256 * it, r = e / SR, x = e - r * SR;
        float v[MAX_C];
        load_pixel<T>(s + (((long)b * SR + y0 + r) * SR + x) * src.cs + src.coff, C, v);
#pragma unroll
        for (int c = 0; c < MAX_C; ++c) {
            if (c < C) {
                bad += (__float_as_uint(v[c]) & 0x7f800000u) == 0x7f800000u;
                // ssr_quantize_u8 mode 1: clamp(0, 1) then * 255 in fp32 (NaN -> 0 via fmaxf), truncation
                bytes[(r * SR + x) * C + c] = (uint8_t)(fminf(fmaxf(v[c], 0.f), 1.f) * 255.0f);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(nonfinite, bad);
    __syncthreads();
    const int row16 = SR * C / 16;                                // uint4 per chunk row of the mosaic
    for (int e = threadIdx.x; e < SROWS * row16; e += 256) {
        const int r = e / row16, q = e - r * row16;
        *reinterpret_cast<uint4*>(mosaic + (((long)ci * SR + y0 + r) * Wo + (long)cj * SR) * C + 16 * q) = img[e];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- chunks at arbitrary places (the overlap-and-blend path) ----
constexpr int ROWB = CH * 3;       // bytes per chunk row of the scene
constexpr int ROWW = ROWB / 4 + 1; // aligned 4-byte words that cover a chunk row starting at any byte

// Word i (<= LEN / 4) of the aligned words covering the LEN bytes at `a` (any alignment; LEN = ROWB for a TCI row, CH for a row of
// a band plane): one word load where the word lies inside the row, single byte loads at its two ends (nothing outside
// [a, a + LEN) is read); bytes outside the row come back as 0xff.  Row byte j sits at byte (a & 3) + j of the words.
template <int LEN>
__device__ __forceinline__ uint32_t row_word(const uint8_t* a, int i) {
    const int sh = (int)(reinterpret_cast<uintptr_t>(a) & 3);
    const int j0 = 4 * i - sh;                                    // row byte index of the word's first byte
    if (j0 >= 0 && j0 + 4 <= LEN) return *reinterpret_cast<const uint32_t*>(a + j0);
    uint32_t v = 0xffffffffu;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j >= 0 && j < LEN) v = (v & ~(0xffu << (8 * u))) | ((uint32_t)a[j] << (8 * u));
    }
    return v;
}

__device__ __forceinline__ bool origin_ok(int y0, int x0, int H, int W) { return y0 >= 0 && x0 >= 0 && y0 <= H - CH && x0 <= W - CH; }

// one wave per (chunk, frame): CH rows x ROWW words, 0xff outside the rows
__global__ __launch_bounds__(256) void scene_zero_scan_at_kernel(const uint8_t* __restrict__ scene, int T, int H, int W,
                                                                 const int32_t* __restrict__ origins, int n_chunks,
                                                                 uint8_t* __restrict__ has_zero) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)n_chunks * T) return;                       // wave-uniform
    const int lane = threadIdx.x & 63;
    const int chunk = (int)(item / T), t = (int)(item - (long)chunk * T);
    const int y0 = origins[2 * chunk], x0 = origins[2 * chunk + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // wave-uniform
    const uint8_t* base = scene + (((long)t * H + y0) * W + x0) * 3;
    bool z = false;
    for (int e = lane; e < CH * ROWW; e += 64) {
        const int row = e / ROWW, i = e - row * ROWW;
        z |= has_zero_byte(row_word<ROWB>(base + (long)row * W * 3, i));
    }
    const bool any = __any(z);
    if (lane == 0) has_zero[item] = any ? 1 : 0;
}

// one block per (chunk, frame): the window's CH rows go through LDS as their covering aligned words (CH x ROWW words, behind them
// the byte offsets of the rows inside their words - 3 W may be odd, so every row has its own), then 4 whole pixels per thread, three
// bytes each wherever they lie in the words.  A pixel counts in z (a zero sample) or in s (all three 255), never in both: one packed
// sum (z << 16) + s, at most 1024 in either half, is the key.  Shuffles inside a wave, one LDS step over the 4 waves.
constexpr int KEYW = CH * ROWW;    // words of a staged window

__global__ __launch_bounds__(256) void scene_frame_keys_kernel(const uint8_t* __restrict__ scene, int T, int H, int W,
                                                               const int32_t* __restrict__ origins, uint32_t* __restrict__ keys) {
    __shared__ uint32_t win[KEYW + CH + 4];                       // [CH][ROWW] words, [CH] byte offsets, the 4 waves' sums
    uint32_t* shift = win + KEYW;
    uint32_t* part = shift + CH;
    const int chunk = blockIdx.x / T, t = blockIdx.x - chunk * T;
    const int y0 = origins[2 * chunk], x0 = origins[2 * chunk + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // block-uniform: before any barrier
    const uint8_t* base = scene + (((long)t * H + y0) * W + x0) * 3;
    for (int e = threadIdx.x; e < KEYW; e += 256) {
        const int row = e / ROWW, i = e - row * ROWW;
        const uint8_t* a = base + (long)row * W * 3;
        win[e] = row_word<ROWB>(a, i);
        if (i == 0) shift[row] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(win);
    uint32_t zs = 0;
#pragma unroll
    for (int k = 0; k < CH * CH / 256; ++k) {
        const int p = threadIdx.x + 256 * k, row = p / CH, x = p - row * CH;
        const uint8_t* px = bytes + row * (4 * ROWW) + shift[row] + 3 * x;
        const uint32_t r = px[0], g = px[1], b = px[2];
        zs += (r == 0 || g == 0 || b == 0) ? 0x10000u : ((r & g & b) == 0xffu ? 1u : 0u);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) zs += __shfl_down(zs, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = zs;
    __syncthreads();
    if (threadIdx.x == 0) keys[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// one wave per chunk (a block of 64): the chunk's T keys in LDS, one lane per frame i (a strided loop beyond 64 frames) counts the
// frames that come before it in the order (key, index) - every lane reads the same word, a broadcast - and, if fewer than n do,
// writes i at that place.  The ranks are a permutation of 0 .. T - 1: every place below n is written exactly once.
constexpr int MAX_T = 1024;        // frames ssr_scene_rank_frames accepts

__global__ __launch_bounds__(64) void scene_rank_frames_kernel(const uint32_t* __restrict__ keys, int T, int n,
                                                               int32_t* __restrict__ frame_ids) {
    __shared__ uint32_t k[MAX_T];
    const long chunk = blockIdx.x;
    for (int i = threadIdx.x; i < T; i += 64) k[i] = keys[chunk * T + i];
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += 64) {
        const uint32_t ki = k[i];
        int rank = 0;
        for (int j = 0; j < T; ++j) {
            const uint32_t kj = k[j];
            rank += (kj < ki) || (kj == ki && j < i);
        }
        if (rank < n) frame_ids[chunk * n + rank] = i;
    }
}

// scene_gather_kernel at an arbitrary origin: the rows go through LDS as their covering aligned words (n x ROWW words, and the n
// byte offsets of the rows inside them), the conversion and the stores are the same
template <typename T, int V>
__global__ __launch_bounds__(256) void scene_gather_at_kernel(const uint8_t* __restrict__ scene, int T_, int H, int W,
                                                              const int32_t* __restrict__ origins,
                                                              const int32_t* __restrict__ frame_ids, int n, ssr_view dst) {
    extern __shared__ uint32_t roww[];                            // [n][ROWW] words, then [n] byte offsets
    uint32_t* shift = roww + n * ROWW;
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // block-uniform
    for (int k = 0; k < n; ++k) {                                 // block-uniform: before any barrier
        const int f = frame_ids[b * n + k];
        if (f < 0 || f >= T_) return;
    }
    for (int e = threadIdx.x; e < n * ROWW; e += 256) {
        const int k = e / ROWW, i = e - k * ROWW;
        const long t = frame_ids[b * n + k];
        const uint8_t* a = scene + ((t * H + y0 + y) * W + x0) * 3;
        roww[e] = row_word<ROWB>(a, i);
        if (i == 0) shift[k] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(roww);
    const int C = 3 * n, groups = C / V;
    T* __restrict__ d = reinterpret_cast<T*>(dst.p);
    const long pix0 = ((long)b * CH + y) * CH;
    for (int e = threadIdx.x; e < CH * groups; e += 256) {
        const int x = e / groups, c0 = (e - x * groups) * V;
        Pack<T, V> o;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int c = c0 + u, k = c / 3;
            // x * (1.0f / 255.0f), then the storage type's rounding: scene_gather_kernel's arithmetic
            o.v[u] = from_f32<T>((float)bytes[k * (4 * ROWW) + shift[k] + x * 3 + (c - 3 * k)] * INV255);
        }
        *reinterpret_cast<Pack<T, V>*>(d + (pix0 + x) * dst.cs + dst.coff + c0) = o;
    }
}

// scene_gather_at_kernel for 3 + K channels per chosen frame: the n TCI rows (n x ROWW words) and the n K rows of the band planes
// (n K x BANDW words, slot-major) go through LDS as their covering aligned words, behind them the byte offsets of the rows inside
// their words.  Channel s (3 + K) + c of a pixel is the TCI sample c < 3 of slot s, else band c - 3.  The row strides (25 and 9
// words) are odd: the byte reads of consecutive channels, which step from one row to the next, spread over the banks.
constexpr int BANDW = CH / 4 + 1;  // aligned 4-byte words that cover a row of a band plane starting at any byte

template <typename T, int V>
__global__ __launch_bounds__(256) void scene_gather_bands_kernel(const uint8_t* __restrict__ tci, const uint8_t* __restrict__ bands,
                                                                 int K, int T_, int H, int W, const int32_t* __restrict__ origins,
                                                                 const int32_t* __restrict__ frame_ids, int n, ssr_view dst) {
    extern __shared__ uint32_t roww[];                            // [n][ROWW], [n K][BANDW] words, then [n] and [n K] byte offsets
    uint32_t* bandw = roww + n * ROWW;
    uint32_t* shift = bandw + n * K * BANDW;
    uint32_t* bshift = shift + n;
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // block-uniform
    for (int s = 0; s < n; ++s) {                                 // block-uniform: before any barrier
        const int f = frame_ids[b * n + s];
        if (f < 0 || f >= T_) return;
    }
    const int tci_words = n * ROWW;
    for (int e = threadIdx.x; e < tci_words + n * K * BANDW; e += 256) {
        if (e < tci_words) {
            const int s = e / ROWW, i = e - s * ROWW;
            const long t = frame_ids[b * n + s];
            const uint8_t* a = tci + ((t * H + y0 + y) * W + x0) * 3;
            roww[e] = row_word<ROWB>(a, i);
            if (i == 0) shift[s] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
        } else {
            const int r = (e - tci_words) / BANDW, i = (e - tci_words) - r * BANDW;      // r = s K + band
            const int s = r / K, kb = r - s * K;
            const long t = frame_ids[b * n + s];
            const uint8_t* a = bands + (((long)kb * T_ + t) * H + y0 + y) * W + x0;
            bandw[r * BANDW + i] = row_word<CH>(a, i);
            if (i == 0) bshift[r] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
        }
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(roww);
    const uint8_t* bbytes = reinterpret_cast<const uint8_t*>(bandw);
    const int F = 3 + K, C = n * F, groups = C / V;
    T* __restrict__ d = reinterpret_cast<T*>(dst.p);
    const long pix0 = ((long)b * CH + y) * CH;
    for (int e = threadIdx.x; e < CH * groups; e += 256) {
        const int x = e / groups, c0 = (e - x * groups) * V;
        int s = c0 / F, c = c0 - s * F;                           // slot and channel inside the slot of the pack's first element
        Pack<T, V> o;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int r = s * K + c - 3;
            const uint8_t v = c < 3 ? bytes[s * (4 * ROWW) + shift[s] + x * 3 + c] : bbytes[r * (4 * BANDW) + bshift[r] + x];
            // x * (1.0f / 255.0f), then the storage type's rounding: scene_gather_kernel's arithmetic
            o.v[u] = from_f32<T>((float)v * INV255);
            if (++c == F) { c = 0; ++s; }
        }
        *reinterpret_cast<Pack<T, V>*>(d + (pix0 + x) * dst.cs + dst.coff + c0) = o;
    }
}

// scene_gather_bands_kernel (K >= 1) and scene_gather_at_kernel (K == 0, bands not read) under a transform of the square: the
// block of SOURCE row y stages the rows exactly as they do - whole rows as aligned words - and converts with the same arithmetic;
// only the place of a pixel in dst turns.  Source pixel (y, x) goes to (yd, xd) = (tf & 2 ? 31 - y : y, tf & 1 ? 31 - x : x), swapped
// if tf & 4: without a transpose the block writes a row of dst (backwards under a column flip), under a transpose a column of it,
// one pixel's channel vector (or V of its channels) per store.  tf outside 0 .. 7: a no-op, block-uniform like the other two.
template <typename T, int V>
__global__ __launch_bounds__(256) void scene_gather_tf_kernel(const uint8_t* __restrict__ tci, const uint8_t* __restrict__ bands,
                                                              int K, int T_, int H, int W, const int32_t* __restrict__ origins,
                                                              const int32_t* __restrict__ frame_ids, const int32_t* __restrict__ tf,
                                                              int n, ssr_view dst) {
    extern __shared__ uint32_t roww[];                            // [n][ROWW], [n K][BANDW] words, then [n] and [n K] byte offsets
    uint32_t* bandw = roww + n * ROWW;
    uint32_t* shift = bandw + n * K * BANDW;
    uint32_t* bshift = shift + n;
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // block-uniform
    const int t8 = tf[b];
    if (t8 < 0 || t8 > 7) return;                                 // block-uniform
    for (int s = 0; s < n; ++s) {                                 // block-uniform: before any barrier
        const int f = frame_ids[b * n + s];
        if (f < 0 || f >= T_) return;
    }
    const int tci_words = n * ROWW;
    for (int e = threadIdx.x; e < tci_words + n * K * BANDW; e += 256) {
        if (e < tci_words) {
            const int s = e / ROWW, i = e - s * ROWW;
            const long t = frame_ids[b * n + s];
            const uint8_t* a = tci + ((t * H + y0 + y) * W + x0) * 3;
            roww[e] = row_word<ROWB>(a, i);
            if (i == 0) shift[s] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
        } else {                                                  // (K >= 1 here)
            const int r = (e - tci_words) / BANDW, i = (e - tci_words) - r * BANDW;      // r = s K + band
            const int s = r / K, kb = r - s * K;
            const long t = frame_ids[b * n + s];
            const uint8_t* a = bands + (((long)kb * T_ + t) * H + y0 + y) * W + x0;
            bandw[r * BANDW + i] = row_word<CH>(a, i);
            if (i == 0) bshift[r] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
        }
    }
    __syncthreads();
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(roww);
    const uint8_t* bbytes = reinterpret_cast<const uint8_t*>(bandw);
    const int F = 3 + K, C = n * F, groups = C / V;
    T* __restrict__ d = reinterpret_cast<T*>(dst.p);
    const int yd = (t8 & 2) ? CH - 1 - y : y;
    for (int e = threadIdx.x; e < CH * groups; e += 256) {
        const int x = e / groups, c0 = (e - x * groups) * V;
        const int xd = (t8 & 1) ? CH - 1 - x : x;
        const int py = (t8 & 4) ? xd : yd, px = (t8 & 4) ? yd : xd;      // both in 0 .. 31
        int s = c0 / F, c = c0 - s * F;                           // slot and channel inside the slot of the pack's first element
        Pack<T, V> o;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const int r = s * K + c - 3;
            const uint8_t v = c < 3 ? bytes[s * (4 * ROWW) + shift[s] + x * 3 + c] : bbytes[r * (4 * BANDW) + bshift[r] + x];
            // x * (1.0f / 255.0f), then the storage type's rounding: scene_gather_kernel's arithmetic
            o.v[u] = from_f32<T>((float)v * INV255);
            if (++c == F) { c = 0; ++s; }
        }
        *reinterpret_cast<Pack<T, V>*>(d + (((long)b * CH + py) * CH + px) * dst.cs + dst.coff + c0) = o;
    }
}

// one wave per (batch item, row of its 128 x 128 output): the row's 128 C fixed-point samples, weighted, are added to 128 C
// consecutive words of the accumulator - wave-instructions of 256 contiguous bytes.  Integer adds: the sums do not depend on the
// order in which overlapping chunks arrive.
template <typename T>
__global__ __launch_bounds__(256) void scene_blend_add_kernel(ssr_view src, const int32_t* __restrict__ origins, int B, int C,
                                                              const int32_t* __restrict__ window, uint32_t* __restrict__ acc,
                                                              int Ho, int Wo, int32_t* __restrict__ nonfinite) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)B * SR) return;                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int b = (int)(item / SR), r = (int)(item - (long)b * SR);
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, Ho / 4, Wo / 4)) return;               // wave-uniform
    const T* __restrict__ s = reinterpret_cast<const T*>(src.p) + ((long)b * SR + r) * SR * src.cs + src.coff;
    uint32_t* __restrict__ a = acc + (((long)4 * y0 + r) * Wo + (long)4 * x0) * C;
    const uint32_t wr = (uint32_t)window[r];
    int bad = 0;
    for (int e = lane; e < SR * C; e += 64) {
        const int x = e / C, c = e - x * C;
        const float v = to_f32(s[(long)x * src.cs + c]);
        bad += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        // clamp(0, 1) (NaN -> 0 via fmaxf) * 65535 in fp32, truncated: 16 fractional bits of the sample
        const uint32_t f = (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * 65535.0f);
        atomicAdd(a + e, f * wr * (uint32_t)window[x]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    if (lane == 0 && bad) atomicAdd(nonfinite, bad);
}

// scene_blend_add_kernel for a (chunk, transform) row of the self-ensemble: the wave that owns accumulator row r of item b adds the
// INVERSE transform of the item's output, so it reads src at the preimage of (r, x) - row rs = tf & 2 ? 127 - r : r and column
// xs = tf & 1 ? 127 - x : x, swapped if tf & 4 (then a column of src: a strided read) - and adds into the same 128 C consecutive
// words: the reads turn, the atomics stay contiguous.  The window is indexed by the place in the accumulator.  13 fractional bits:
// 8 rows per chunk x 125 x 125 (the largest weight sums) x 8191 < 2^32.  tf outside 0 .. 7: a no-op, wave-uniform.
constexpr float ENS_ONE = 8191.0f;

template <typename T>
__global__ __launch_bounds__(256) void scene_blend_add_tf_kernel(ssr_view src, const int32_t* __restrict__ origins,
                                                                 const int32_t* __restrict__ tf, int B, int C,
                                                                 const int32_t* __restrict__ window, uint32_t* __restrict__ acc,
                                                                 int Ho, int Wo, int32_t* __restrict__ nonfinite) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)B * SR) return;                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int b = (int)(item / SR), r = (int)(item - (long)b * SR);
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, Ho / 4, Wo / 4)) return;               // wave-uniform
    const int t8 = tf[b];
    if (t8 < 0 || t8 > 7) return;                                 // wave-uniform
    const T* __restrict__ s = reinterpret_cast<const T*>(src.p) + (long)b * SR * SR * src.cs + src.coff;
    uint32_t* __restrict__ a = acc + (((long)4 * y0 + r) * Wo + (long)4 * x0) * C;
    const uint32_t wr = (uint32_t)window[r];
    const int rs = (t8 & 2) ? SR - 1 - r : r;
    int bad = 0;
    for (int e = lane; e < SR * C; e += 64) {
        const int x = e / C, c = e - x * C;
        const int xs = (t8 & 1) ? SR - 1 - x : x;
        const int pix = (t8 & 4) ? xs * SR + rs : rs * SR + xs;  // below 128 * 128
        const float v = to_f32(s[(long)pix * src.cs + c]);
        bad += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        // clamp(0, 1) (NaN -> 0 via fmaxf) * 8191 in fp32, truncated: 13 fractional bits of the sample
        const uint32_t f = (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * ENS_ONE);
        atomicAdd(a + e, f * wr * (uint32_t)window[x]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    if (lane == 0 && bad) atomicAdd(nonfinite, bad);
}

// one thread per aligned 4-byte unit of the mosaic (a row is Wo C bytes, Wo a multiple of 4); `scale` is the fixed point's one
// times the rows per chunk: the constant 65535 in scene_blend_finish_kernel, an argument in scene_blend_finish_scaled_kernel
__device__ __forceinline__ void blend_finish_unit(const uint32_t* __restrict__ acc, const int32_t* __restrict__ Sy,
                                                  const int32_t* __restrict__ Sx, int C, uint32_t* __restrict__ mosaic, int Ho, int Wo,
                                                  uint32_t scale) {
    const long roww_ = (long)Wo * C / 4;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= roww_ * Ho) return;
    const int y = (int)(q / roww_);
    const int j0 = (int)(q - (long)y * roww_) * 4;                // first byte of the unit inside its row
    const uint64_t sy = (uint64_t)Sy[y] * scale;
    const u32x4 a4 = *reinterpret_cast<const u32x4*>(acc + 4 * q);   // the unit's 4 samples: 16 aligned bytes
    uint32_t out = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int x = (j0 + u) / C;
        const uint64_t den = sy * (uint64_t)Sx[x];
        const uint64_t num = (uint64_t)a4[u] * 255u;
        out |= (uint32_t)(den ? (num / den) & 0xff : 0) << (8 * u);
    }
    mosaic[q] = out;
}

__global__ __launch_bounds__(256) void scene_blend_finish_kernel(const uint32_t* __restrict__ acc, const int32_t* __restrict__ Sy,
                                                                 const int32_t* __restrict__ Sx, int C, uint32_t* __restrict__ mosaic,
                                                                 int Ho, int Wo) {
    blend_finish_unit(acc, Sy, Sx, C, mosaic, Ho, Wo, 65535u);
}

__global__ __launch_bounds__(256) void scene_blend_finish_scaled_kernel(const uint32_t* __restrict__ acc, const int32_t* __restrict__ Sy,
                                                                        const int32_t* __restrict__ Sx, int C, uint32_t scale,
                                                                        uint32_t* __restrict__ mosaic, int Ho, int Wo) {
    blend_finish_unit(acc, Sy, Sx, C, mosaic, Ho, Wo, scale);
}

// one block per (chunk, row of its window): the n chosen frames' rows go through LDS as their covering aligned words, exactly as
// scene_gather_at_kernel stages them (the same no-op tests, so support counts what the gather fed to the generator), then one
// thread per pixel of the row counts the slots whose three samples are all non-zero and adds the count to the pixel's word of
// support.  Integer atomics: overlapping chunks may arrive in any order.
__global__ __launch_bounds__(256) void scene_support_add_kernel(const uint8_t* __restrict__ scene, int T_, int H, int W,
                                                                const int32_t* __restrict__ origins,
                                                                const int32_t* __restrict__ frame_ids, int n,
                                                                int32_t* __restrict__ support) {
    extern __shared__ uint32_t roww[];                            // [n][ROWW] words, then [n] byte offsets
    uint32_t* shift = roww + n * ROWW;
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, H, W)) return;                         // block-uniform
    for (int k = 0; k < n; ++k) {                                 // block-uniform: before any barrier
        const int f = frame_ids[b * n + k];
        if (f < 0 || f >= T_) return;
    }
    for (int e = threadIdx.x; e < n * ROWW; e += 256) {
        const int k = e / ROWW, i = e - k * ROWW;
        const long t = frame_ids[b * n + k];
        const uint8_t* a = scene + ((t * H + y0 + y) * W + x0) * 3;
        roww[e] = row_word<ROWB>(a, i);
        if (i == 0) shift[k] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
    }
    __syncthreads();
    if (threadIdx.x >= CH) return;                                // (after the only barrier)
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(roww);
    const int x = threadIdx.x;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const uint8_t* px = bytes + k * (4 * ROWW) + shift[k] + 3 * x;
        count += (px[0] != 0) & (px[1] != 0) & (px[2] != 0);
    }
    if (count) atomicAdd(support + (long)(y0 + y) * W + x0 + x, count);
}

// one thread per aligned 4-byte unit of the mosaic (a row is Wo C bytes, Wo a multiple of 4), as scene_blend_finish_kernel stores:
// for C = 3 a unit spans two output pixels, which can belong to two low-resolution pixels, so the rule is decided per byte.  The
// thread that holds the first byte of a low-resolution pixel's 4 x 4 block also writes the pixel's saturated support.
__global__ __launch_bounds__(256) void scene_apply_nodata_kernel(uint32_t* __restrict__ mosaic, int Ho, int Wo, int C,
                                                                 const int32_t* __restrict__ support, int min_support,
                                                                 uint8_t* __restrict__ support_u8) {
    const long roww_ = (long)Wo * C / 4;
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    if (q >= roww_ * Ho) return;
    const int y = (int)(q / roww_);
    const int j0 = (int)(q - (long)y * roww_) * 4;                // first byte of the unit inside its row
    const int W = Wo / 4;
    const int32_t* __restrict__ srow = support + (long)(y >> 2) * W;
    int x = j0 / C, c = j0 - x * C;                               // output pixel and channel of the unit's first byte
    const uint32_t in = mosaic[q];
    uint32_t out = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int s = srow[x >> 2];
        const uint32_t v = (in >> (8 * u)) & 0xffu;
        out |= (s < min_support ? 0u : (v ? v : 1u)) << (8 * u);
        if (support_u8 && c == 0 && (x & 3) == 0 && (y & 3) == 0)
            support_u8[(long)(y >> 2) * W + (x >> 2)] = (uint8_t)(s > 255 ? 255 : s);
        if (++c == C) { c = 0; ++x; }
    }
    mosaic[q] = out;
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_scene_zero_scan(const uint8_t* scene, int32_t T, int32_t H, int32_t W, uint8_t* has_zero, void* stream) {
    if (!scene || !has_zero || T <= 0 || H <= 0 || W <= 0 || !aligned16(scene)) return SSR_EINVAL;
    if (H % CH || W % CH) return SSR_EUNSUP;
    const long items = (long)(H / CH) * (W / CH) * T;
    if (items > (1l << 30)) return SSR_EINVAL;
    hipLaunchKernelGGL(scene_zero_scan_kernel, dim3((int)((items + 3) / 4)), dim3(256), 0, ST(stream), scene, T, H, W, has_zero);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_gather(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* chunk_ids,
                                const int32_t* frame_ids, int32_t B, int32_t n, ssr_view dst, int32_t dtype, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!scene || !chunk_ids || !frame_ids || !dst.p || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0) return SSR_EINVAL;
    if (!aligned16(scene) || !aligned16(dst.p) || dst.cs % 8 || dst.coff % 8 || dst.coff < 0 || dst.coff + 3 * n > dst.cs ||
        B > (1 << 20))
        return SSR_EINVAL;
    if (H % CH || W % CH || n > T || n > 512 || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * CH), block(256);
    const size_t lds = (size_t)n * CH * 3;
    const int C = 3 * n;
    if (dtype == SSR_F32) {
        if (C % 4 == 0)
            hipLaunchKernelGGL((scene_gather_kernel<float, 4>), grid, block, lds, ST(stream), scene, T, H, W, chunk_ids, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_kernel<float, 1>), grid, block, lds, ST(stream), scene, T, H, W, chunk_ids, frame_ids, n, dst);
    } else {
        if (C % 8 == 0)
            hipLaunchKernelGGL((scene_gather_kernel<__bf16, 8>), grid, block, lds, ST(stream), scene, T, H, W, chunk_ids, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_kernel<__bf16, 1>), grid, block, lds, ST(stream), scene, T, H, W, chunk_ids, frame_ids, n, dst);
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_scatter_u8(ssr_view src, int32_t dtype, const int32_t* chunk_ids, int32_t B, int32_t C, uint8_t* mosaic,
                                    int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!src.p || !chunk_ids || !mosaic || !nonfinite || B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    // whole pixels are read: the 8 channels from coff on must lie inside the buffer's pixel
    if (!aligned16(src.p) || !aligned16(mosaic) || src.cs % 8 || src.coff % 8 || src.coff < 0 || src.coff + MAX_C > src.cs ||
        C > MAX_C || B > (1 << 20))
        return SSR_EINVAL;
    if (Ho % SR || Wo % SR || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * (SR / SROWS)), block(256);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(scene_scatter_u8_kernel<float>, grid, block, 0, ST(stream), src, chunk_ids, C, mosaic, Ho, Wo, nonfinite);
    else
        hipLaunchKernelGGL(scene_scatter_u8_kernel<__bf16>, grid, block, 0, ST(stream), src, chunk_ids, C, mosaic, Ho, Wo, nonfinite);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_zero_scan_at(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, int32_t n_chunks,
                                      uint8_t* has_zero, void* stream) {
    if (!scene || !origins || !has_zero || T <= 0 || H <= 0 || W <= 0 || n_chunks <= 0) return SSR_EINVAL;
    if (H < CH || W < CH) return SSR_EUNSUP;
    const long items = (long)n_chunks * T;
    if (items > (1l << 30)) return SSR_EINVAL;
    hipLaunchKernelGGL(scene_zero_scan_at_kernel, dim3((int)((items + 3) / 4)), dim3(256), 0, ST(stream), scene, T, H, W, origins,
                       n_chunks, has_zero);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_gather_at(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins,
                                   const int32_t* frame_ids, int32_t B, int32_t n, ssr_view dst, int32_t dtype, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!scene || !origins || !frame_ids || !dst.p || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0) return SSR_EINVAL;
    if (!aligned16(dst.p) || dst.cs % 8 || dst.coff % 8 || dst.coff < 0 || dst.coff + 3 * n > dst.cs || B > (1 << 20))
        return SSR_EINVAL;
    if (H < CH || W < CH || n > T || n > 512 || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * CH), block(256);
    const size_t lds = (size_t)n * (ROWW + 1) * 4;
    const int C = 3 * n;
    if (dtype == SSR_F32) {
        if (C % 4 == 0)
            hipLaunchKernelGGL((scene_gather_at_kernel<float, 4>), grid, block, lds, ST(stream), scene, T, H, W, origins, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_at_kernel<float, 1>), grid, block, lds, ST(stream), scene, T, H, W, origins, frame_ids, n, dst);
    } else {
        if (C % 8 == 0)
            hipLaunchKernelGGL((scene_gather_at_kernel<__bf16, 8>), grid, block, lds, ST(stream), scene, T, H, W, origins, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_at_kernel<__bf16, 1>), grid, block, lds, ST(stream), scene, T, H, W, origins, frame_ids, n, dst);
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_gather_bands(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W,
                                      const int32_t* origins, const int32_t* frame_ids, int32_t B, int32_t n, ssr_view dst,
                                      int32_t dtype, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!tci || !bands || !origins || !frame_ids || !dst.p || K <= 0 || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0) return SSR_EINVAL;
    const long C = (long)n * (3 + (long)K);
    if (!aligned16(dst.p) || dst.cs % 8 || dst.coff % 8 || dst.coff < 0 || dst.coff + C > dst.cs || B > (1 << 20)) return SSR_EINVAL;
    const size_t lds = ((size_t)n * (ROWW + 1) + (size_t)n * K * (BANDW + 1)) * 4;
    if (H < CH || W < CH || n > T || n > 512 || lds > 65536 || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * CH), block(256);
    if (dtype == SSR_F32) {
        if (C % 4 == 0)
            hipLaunchKernelGGL((scene_gather_bands_kernel<float, 4>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_bands_kernel<float, 1>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, n, dst);
    } else {
        if (C % 8 == 0)
            hipLaunchKernelGGL((scene_gather_bands_kernel<__bf16, 8>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_bands_kernel<__bf16, 1>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, n, dst);
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_frame_keys(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins, int32_t n_chunks,
                                    uint32_t* keys, void* stream) {
    if (!scene || !origins || !keys || T <= 0 || H <= 0 || W <= 0 || n_chunks <= 0 || !aligned4(keys)) return SSR_EINVAL;
    if (H < CH || W < CH) return SSR_EUNSUP;
    const long items = (long)n_chunks * T;
    if (items > (1l << 30)) return SSR_EINVAL;
    hipLaunchKernelGGL(scene_frame_keys_kernel, dim3((int)items), dim3(256), 0, ST(stream), scene, T, H, W, origins, keys);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_rank_frames(const uint32_t* keys, int32_t n_chunks, int32_t T, int32_t n, int32_t* frame_ids, void* stream) {
    if (!keys || !frame_ids || n_chunks <= 0 || T <= 0 || n <= 0 || !aligned4(keys) || !aligned4(frame_ids)) return SSR_EINVAL;
    if (T > MAX_T || n > T) return SSR_EUNSUP;
    if ((long)n_chunks * T > (1l << 30)) return SSR_EINVAL;
    hipLaunchKernelGGL(scene_rank_frames_kernel, dim3(n_chunks), dim3(64), 0, ST(stream), keys, T, n, frame_ids);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_blend_add(ssr_view src, int32_t dtype, const int32_t* origins, int32_t B, int32_t C, const int32_t* window,
                                   uint32_t* acc, int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!src.p || !origins || !window || !acc || !nonfinite || B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned4(src.p) || !aligned16(acc) || src.coff < 0 || src.coff + C > src.cs || C > MAX_C || B > (1 << 20)) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * (SR / 4)), block(256);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(scene_blend_add_kernel<float>, grid, block, 0, ST(stream), src, origins, B, C, window, acc, Ho, Wo, nonfinite);
    else
        hipLaunchKernelGGL(scene_blend_add_kernel<__bf16>, grid, block, 0, ST(stream), src, origins, B, C, window, acc, Ho, Wo, nonfinite);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_blend_finish(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, uint8_t* mosaic, int32_t Ho,
                                      int32_t Wo, void* stream) {
    if (!acc || !Sy || !Sx || !mosaic || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned16(acc) || !aligned4(mosaic) || C > MAX_C) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR) return SSR_EUNSUP;
    const long units = (long)Ho * Wo * C / 4, blocks = (units + 255) / 256;
    if (blocks > 0x7fffffffl) return SSR_EUNSUP;
    hipLaunchKernelGGL(scene_blend_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), acc, Sy, Sx, C,
                       reinterpret_cast<uint32_t*>(mosaic), Ho, Wo);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_gather_tf(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W,
                                   const int32_t* origins, const int32_t* frame_ids, const int32_t* tf, int32_t B, int32_t n,
                                   ssr_view dst, int32_t dtype, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!tci || !origins || !frame_ids || !tf || !dst.p || K < 0 || (K > 0 && !bands) || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0)
        return SSR_EINVAL;
    const long C = (long)n * (3 + (long)K);
    if (!aligned16(dst.p) || dst.cs % 8 || dst.coff % 8 || dst.coff < 0 || dst.coff + C > dst.cs || B > (1 << 20)) return SSR_EINVAL;
    const size_t lds = ((size_t)n * (ROWW + 1) + (size_t)n * K * (BANDW + 1)) * 4;
    if (H < CH || W < CH || n > T || n > 512 || lds > 65536 || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * CH), block(256);
    if (dtype == SSR_F32) {
        if (C % 4 == 0)
            hipLaunchKernelGGL((scene_gather_tf_kernel<float, 4>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, tf, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_tf_kernel<float, 1>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, tf, n, dst);
    } else {
        if (C % 8 == 0)
            hipLaunchKernelGGL((scene_gather_tf_kernel<__bf16, 8>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, tf, n, dst);
        else
            hipLaunchKernelGGL((scene_gather_tf_kernel<__bf16, 1>), grid, block, lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, tf, n, dst);
    }
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_blend_add_tf(ssr_view src, int32_t dtype, const int32_t* origins, const int32_t* tf, int32_t B, int32_t C,
                                      const int32_t* window, uint32_t* acc, int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!src.p || !origins || !tf || !window || !acc || !nonfinite || B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned4(src.p) || !aligned16(acc) || src.coff < 0 || src.coff + C > src.cs || C > MAX_C || B > (1 << 20)) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const dim3 grid(B * (SR / 4)), block(256);
    if (dtype == SSR_F32)
        hipLaunchKernelGGL(scene_blend_add_tf_kernel<float>, grid, block, 0, ST(stream), src, origins, tf, B, C, window, acc, Ho, Wo, nonfinite);
    else
        hipLaunchKernelGGL(scene_blend_add_tf_kernel<__bf16>, grid, block, 0, ST(stream), src, origins, tf, B, C, window, acc, Ho, Wo, nonfinite);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_blend_finish_scaled(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, int32_t scale,
                                             uint8_t* mosaic, int32_t Ho, int32_t Wo, void* stream) {
    if (!acc || !Sy || !Sx || !mosaic || C <= 0 || scale < 1 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned16(acc) || !aligned4(mosaic) || C > MAX_C) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR) return SSR_EUNSUP;
    const long units = (long)Ho * Wo * C / 4, blocks = (units + 255) / 256;
    if (blocks > 0x7fffffffl) return SSR_EUNSUP;
    hipLaunchKernelGGL(scene_blend_finish_scaled_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), acc, Sy, Sx, C,
                       (uint32_t)scale, reinterpret_cast<uint32_t*>(mosaic), Ho, Wo);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_support_add(const uint8_t* scene, int32_t T, int32_t H, int32_t W, const int32_t* origins,
                                     const int32_t* frame_ids, int32_t B, int32_t n, int32_t* support, void* stream) {
    if (!scene || !origins || !frame_ids || !support || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0) return SSR_EINVAL;
    if (!aligned4(support) || B > (1 << 20)) return SSR_EINVAL;
    if (H < CH || W < CH || n > T || n > 512) return SSR_EUNSUP;
    const size_t lds = (size_t)n * (ROWW + 1) * 4;
    hipLaunchKernelGGL(scene_support_add_kernel, dim3(B * CH), dim3(256), lds, ST(stream), scene, T, H, W, origins, frame_ids, n,
                       support);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_scene_apply_nodata(uint8_t* mosaic, int32_t Ho, int32_t Wo, int32_t C, const int32_t* support,
                                      int32_t min_support, uint8_t* support_u8, void* stream) {
    if (!mosaic || !support || C <= 0 || Ho <= 0 || Wo <= 0 || min_support < 1) return SSR_EINVAL;
    if (!aligned4(mosaic) || !aligned4(support) || C > MAX_C) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4) return SSR_EUNSUP;
    const long units = (long)Ho * Wo * C / 4, blocks = (units + 255) / 256;
    if (blocks > 0x7fffffffl) return SSR_EUNSUP;
    hipLaunchKernelGGL(scene_apply_nodata_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream),
                       reinterpret_cast<uint32_t*>(mosaic), Ho, Wo, C, support, min_support, support_u8);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
