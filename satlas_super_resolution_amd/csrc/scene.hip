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
//
// The kernels behind the fifteen entry points:
//
//   scene_zero_scan_kernel, scene_gather_kernel<T, V>, scene_scatter_u8_kernel<T>      the grid path's own, aligned 16-byte accesses
//   scene_zero_scan_at_kernel, scene_frame_keys_kernel, scene_rank_frames_kernel, scene_apply_nodata_kernel      one entry point each
//   scene_gather_at_kernel<T, V, BANDS, TF>   ssr_scene_gather_at <.., false, false>, ssr_scene_gather_bands <.., true, false>,
//                                             ssr_scene_gather_tf <.., true, true> (host side: gather_at, pick_pack)
//   scene_support_add_kernel                  ssr_scene_support_add; it and the gather above stage a chunk's rows with stage_rows
//   scene_blend_add_kernel<T, TF>             ssr_scene_blend_add <T, false>, ssr_scene_blend_add_tf <T, true> (host side: blend_add)
//   scene_blend_finish_kernel                 ssr_scene_blend_finish with the scale 65535, ssr_scene_blend_finish_scaled (host side:
//                                             blend_finish)
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

// staging of a row through LDS: word i of the row at `a` to *word and, once per row, the row's byte offset inside its words to *shift
template <int LEN>
__device__ __forceinline__ void stage_word(const uint8_t* a, int i, uint32_t* word, uint32_t* shift) {
    *word = row_word<LEN>(a, i);
    if (i == 0) *shift = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
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
        stage_word<ROWB>(base + (long)row * W * 3, i, win + e, shift + row);
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

// Row y of the window of chunk b, once per chosen frame, through LDS: the n TCI rows as their covering aligned words (n x ROWW) and,
// with BANDS, the n K rows of the band planes (n K x BANDW words, slot-major, r = s K + band), behind them the byte offsets of the
// rows inside their words - the dynamic LDS is [n][ROWW], [n K][BANDW], [n], [n K].  The row strides (25 and 9 words) are odd: the
// byte reads of consecutive channels, which step from one row to the next, spread over the banks.  False, with nothing read or
// staged, for a chunk that is a no-op: its origin outside the scene or a frame id outside 0 .. T - 1 - block-uniform, before the
// barrier.  Every kernel that reads a chunk's rows at an origin stages them here, so what scene_support_add_kernel counts is what
// the gather fed to the generator.
constexpr int BANDW = CH / 4 + 1;  // aligned 4-byte words that cover a row of a band plane starting at any byte

struct StagedRows {
    const uint8_t *bytes, *bbytes;     // the TCI and the band words, read as bytes
    const uint32_t *shift, *bshift;    // per TCI row s and band row r: row byte j is byte shift + j of the row's words
    int y0, x0;                        // the window's origin
};

template <bool BANDS>
__device__ __forceinline__ bool stage_rows(const uint8_t* tci, const uint8_t* bands, int K, int T_, int H, int W,
                                           const int32_t* origins, const int32_t* frame_ids, int n, int b, int y, StagedRows& st) {
    extern __shared__ uint32_t roww[];
    if (!BANDS) K = 0;                                            // (no band rows: the layout is [n][ROWW], [n])
    uint32_t* bandw = roww + n * ROWW;
    uint32_t* shift = bandw + n * K * BANDW;
    uint32_t* bshift = shift + n;
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, H, W)) return false;                   // block-uniform
    for (int s = 0; s < n; ++s) {                                 // block-uniform: before the barrier
        const int f = frame_ids[b * n + s];
        if (f < 0 || f >= T_) return false;
    }
    const int tci_words = n * ROWW;
    for (int e = threadIdx.x; e < tci_words + n * K * BANDW; e += 256) {
        if (!BANDS || e < tci_words) {
            const int s = e / ROWW, i = e - s * ROWW;
            const long t = frame_ids[b * n + s];
            stage_word<ROWB>(tci + ((t * H + y0 + y) * W + x0) * 3, i, roww + e, shift + s);
        } else if constexpr (BANDS) {                             // (K >= 1 here)
            const int r = (e - tci_words) / BANDW, i = (e - tci_words) - r * BANDW;
            const int s = r / K, kb = r - s * K;
            const long t = frame_ids[b * n + s];
            stage_word<CH>(bands + (((long)kb * T_ + t) * H + y0 + y) * W + x0, i, bandw + r * BANDW + i, bshift + r);
        }
    }
    __syncthreads();
    st = {reinterpret_cast<const uint8_t*>(roww), reinterpret_cast<const uint8_t*>(bandw), shift, bshift, y0, x0};
    return true;
}

// scene_gather_kernel at the origins (ssr_scene_gather_at: BANDS and TF off), with 3 + K channels per chosen frame (ssr_scene_gather_bands:
// BANDS; channel s (3 + K) + c of a pixel is the TCI sample c < 3 of slot s, else band c - 3) and under a transform of the square
// (ssr_scene_gather_tf: BANDS and TF, K >= 0 at run time).  One block per (batch item, SOURCE row y): the rows staged by stage_rows,
// the conversion and the stores of scene_gather_kernel; only the place of a pixel in dst turns under TF.  Source pixel (y, x) goes
// to (yd, xd) = (tf & 2 ? 31 - y : y, tf & 1 ? 31 - x : x), swapped if tf & 4: without a transpose the block writes a row of dst
// (backwards under a column flip), under a transpose a column of it, one pixel's channel vector (or V of its channels) per store.
// tf outside 0 .. 7: a no-op, block-uniform like stage_rows' two.
template <typename T, int V, bool BANDS, bool TF>
__global__ __launch_bounds__(256) void scene_gather_at_kernel(const uint8_t* __restrict__ tci, const uint8_t* __restrict__ bands,
                                                              int K, int T_, int H, int W, const int32_t* __restrict__ origins,
                                                              const int32_t* __restrict__ frame_ids, const int32_t* __restrict__ tf,
                                                              int n, ssr_view dst) {
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    int t8 = 0;
    if constexpr (TF) {
        t8 = tf[b];
        if (t8 < 0 || t8 > 7) return;                             // block-uniform
    }
    StagedRows st;
    if (!stage_rows<BANDS>(tci, bands, K, T_, H, W, origins, frame_ids, n, b, y, st)) return;
    const int F = BANDS ? 3 + K : 3, C = n * F, groups = C / V;
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
            const uint8_t v = !BANDS || c < 3 ? st.bytes[s * (4 * ROWW) + st.shift[s] + x * 3 + c]
                                              : st.bbytes[r * (4 * BANDW) + st.bshift[r] + x];
            // `.float() / 255` of frames_to_input: x * (1.0f / 255.0f), then the storage type's rounding (scene_gather_kernel's arithmetic)
            o.v[u] = from_f32<T>((float)v * INV255);
            if (++c == F) { c = 0; ++s; }
        }
        *reinterpret_cast<Pack<T, V>*>(d + (((long)b * CH + py) * CH + px) * dst.cs + dst.coff + c0) = o;
    }
}

// one wave per (batch item, row of its 128 x 128 output): the row's 128 C fixed-point samples, weighted, are added to 128 C
// consecutive words of the accumulator - wave-instructions of 256 contiguous bytes.  Integer adds: the sums do not depend on the
// order in which overlapping chunks arrive.  16 fractional bits of the sample.
// TF (ssr_scene_blend_add_tf), for a (chunk, transform) row of the self-ensemble: the wave that owns accumulator row r of item b adds
// the INVERSE transform of the item's output, so it reads src at the preimage of (r, x) - row rs = tf & 2 ? 127 - r : r and column
// xs = tf & 1 ? 127 - x : x, swapped if tf & 4 (then a column of src: a strided read) - and adds into the same 128 C consecutive
// words: the reads turn, the atomics stay contiguous.  The window is indexed by the place in the accumulator.  13 fractional bits:
// 8 rows per chunk x 125 x 125 (the largest weight sums) x 8191 < 2^32.  tf outside 0 .. 7: a no-op, wave-uniform.
template <typename T, bool TF>
__global__ __launch_bounds__(256) void scene_blend_add_kernel(ssr_view src, const int32_t* __restrict__ origins,
                                                              const int32_t* __restrict__ tf, int B, int C,
                                                              const int32_t* __restrict__ window, uint32_t* __restrict__ acc,
                                                              int Ho, int Wo, int32_t* __restrict__ nonfinite) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)B * SR) return;                             // wave-uniform
    const int lane = threadIdx.x & 63;
    const int b = (int)(item / SR), r = (int)(item - (long)b * SR);
    const int y0 = origins[2 * b], x0 = origins[2 * b + 1];
    if (!origin_ok(y0, x0, Ho / 4, Wo / 4)) return;               // wave-uniform
    int t8 = 0;
    if constexpr (TF) {
        t8 = tf[b];
        if (t8 < 0 || t8 > 7) return;                             // wave-uniform
    }
    // the item's output under TF, which turns the reads; without it row r of the output
    const T* __restrict__ s = reinterpret_cast<const T*>(src.p) + ((long)b * SR + (TF ? 0 : r)) * SR * src.cs + src.coff;
    uint32_t* __restrict__ a = acc + (((long)4 * y0 + r) * Wo + (long)4 * x0) * C;
    const uint32_t wr = (uint32_t)window[r];
    const int rs = (t8 & 2) ? SR - 1 - r : r;
    constexpr float ONE = TF ? 8191.0f : 65535.0f;                // 1.0 in the accumulator's fixed point
    int bad = 0;
    for (int e = lane; e < SR * C; e += 64) {
        const int x = e / C, c = e - x * C;
        const int xs = (t8 & 1) ? SR - 1 - x : x;
        const int pix = !TF ? x : (t8 & 4) ? xs * SR + rs : rs * SR + xs;      // below 128 * 128
        const float v = to_f32(s[(long)pix * src.cs + c]);
        bad += (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
        // clamp(0, 1) (NaN -> 0 via fmaxf) * ONE in fp32, truncated
        const uint32_t f = (uint32_t)(fminf(fmaxf(v, 0.f), 1.f) * ONE);
        atomicAdd(a + e, f * wr * (uint32_t)window[x]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_down(bad, o, 64);
    if (lane == 0 && bad) atomicAdd(nonfinite, bad);
}

// one thread per aligned 4-byte unit of the mosaic (a row is Wo C bytes, Wo a multiple of 4); `scale` is the fixed point's one
// times the rows per chunk: 65535 behind scene_blend_add_kernel<T, false>, 8 * 8191 behind the self-ensemble's
__global__ __launch_bounds__(256) void scene_blend_finish_kernel(const uint32_t* __restrict__ acc, const int32_t* __restrict__ Sy,
                                                                 const int32_t* __restrict__ Sx, int C, uint32_t scale,
                                                                 uint32_t* __restrict__ mosaic, int Ho, int Wo) {
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

// one block per (chunk, row of its window): the n chosen frames' rows staged by stage_rows, as the gather beside it stages them,
// then one thread per pixel of the row counts the slots whose three samples are all non-zero and adds the count to the pixel's word
// of support.  Integer atomics: overlapping chunks may arrive in any order.
__global__ __launch_bounds__(256) void scene_support_add_kernel(const uint8_t* __restrict__ scene, int T_, int H, int W,
                                                                const int32_t* __restrict__ origins,
                                                                const int32_t* __restrict__ frame_ids, int n,
                                                                int32_t* __restrict__ support) {
    const int b = blockIdx.x / CH, y = blockIdx.x - b * CH;
    StagedRows st;
    if (!stage_rows<false>(scene, nullptr, 0, T_, H, W, origins, frame_ids, n, b, y, st)) return;
    if (threadIdx.x >= CH) return;                                // (after the only barrier)
    const int x = threadIdx.x;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const uint8_t* px = st.bytes + k * (4 * ROWW) + st.shift[k] + 3 * x;
        count += (px[0] != 0) & (px[1] != 0) & (px[2] != 0);
    }
    if (count) atomicAdd(support + (long)(st.y0 + y) * W + st.x0 + x, count);
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

#define ST(s) reinterpret_cast<hipStream_t>(s)

// the gathers' launch switch: storage type x vector width V (16 bytes of channels per store when a pixel's C channels are a
// multiple of that, else single elements); the four instantiations of a gather have one signature
template <typename Kernel>
Kernel pick_pack(int dtype, long C, Kernel f32x4, Kernel f32x1, Kernel bf16x8, Kernel bf16x1) {
    return dtype == SSR_F32 ? (C % 4 == 0 ? f32x4 : f32x1) : (C % 8 == 0 ? bf16x8 : bf16x1);
}

// ssr_scene_gather_at (K = 0), ssr_scene_gather_bands and ssr_scene_gather_tf behind their own checks of bands, K and tf: the
// checks the three share, in their order, and the launch
template <bool BANDS, bool TF>
int gather_at(const uint8_t* tci, const uint8_t* bands, int K, int T, int H, int W, const int32_t* origins, const int32_t* frame_ids,
              const int32_t* tf, int B, int n, ssr_view dst, int dtype, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!tci || !origins || !frame_ids || !dst.p || T <= 0 || H <= 0 || W <= 0 || B <= 0 || n <= 0) return SSR_EINVAL;
    const long C = (long)n * (3 + (long)K);
    if (!aligned16(dst.p) || dst.cs % 8 || dst.coff % 8 || dst.coff < 0 || dst.coff + C > dst.cs || B > (1 << 20)) return SSR_EINVAL;
    const size_t lds = ((size_t)n * (ROWW + 1) + (size_t)n * K * (BANDW + 1)) * 4;
    if (H < CH || W < CH || n > T || n > 512 || lds > 65536 || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const auto kernel = pick_pack(dtype, C, scene_gather_at_kernel<float, 4, BANDS, TF>, scene_gather_at_kernel<float, 1, BANDS, TF>,
                                  scene_gather_at_kernel<__bf16, 8, BANDS, TF>, scene_gather_at_kernel<__bf16, 1, BANDS, TF>);
    hipLaunchKernelGGL(kernel, dim3(B * CH), dim3(256), lds, ST(stream), tci, bands, K, T, H, W, origins, frame_ids, tf, n, dst);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

// ssr_scene_blend_add and, behind its own check of tf, ssr_scene_blend_add_tf
template <bool TF>
int blend_add(ssr_view src, int dtype, const int32_t* origins, const int32_t* tf, int B, int C, const int32_t* window, uint32_t* acc,
              int Ho, int Wo, int32_t* nonfinite, void* stream) {
    if (dtype == SSR_F32X3) dtype = SSR_F32;   // fp32 storage: only the matrix-core kernels differ
    if (!src.p || !origins || !window || !acc || !nonfinite || B <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned4(src.p) || !aligned16(acc) || src.coff < 0 || src.coff + C > src.cs || C > MAX_C || B > (1 << 20)) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR || (dtype != SSR_F32 && dtype != SSR_BF16)) return SSR_EUNSUP;
    const auto kernel = dtype == SSR_F32 ? scene_blend_add_kernel<float, TF> : scene_blend_add_kernel<__bf16, TF>;
    hipLaunchKernelGGL(kernel, dim3(B * (SR / 4)), dim3(256), 0, ST(stream), src, origins, tf, B, C, window, acc, Ho, Wo, nonfinite);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

// ssr_scene_blend_finish (scale 65535) and, behind its own check of scale, ssr_scene_blend_finish_scaled
int blend_finish(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int C, uint32_t scale, uint8_t* mosaic, int Ho, int Wo,
                 void* stream) {
    if (!acc || !Sy || !Sx || !mosaic || C <= 0 || Ho <= 0 || Wo <= 0) return SSR_EINVAL;
    if (!aligned16(acc) || !aligned4(mosaic) || C > MAX_C) return SSR_EINVAL;
    if (Ho % 4 || Wo % 4 || Ho < SR || Wo < SR) return SSR_EUNSUP;
    const long units = (long)Ho * Wo * C / 4, blocks = (units + 255) / 256;
    if (blocks > 0x7fffffffl) return SSR_EUNSUP;
    hipLaunchKernelGGL(scene_blend_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, ST(stream), acc, Sy, Sx, C, scale,
                       reinterpret_cast<uint32_t*>(mosaic), Ho, Wo);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

}  // namespace

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
    const auto kernel = pick_pack(dtype, 3 * n, scene_gather_kernel<float, 4>, scene_gather_kernel<float, 1>,
                                  scene_gather_kernel<__bf16, 8>, scene_gather_kernel<__bf16, 1>);
    hipLaunchKernelGGL(kernel, dim3(B * CH), dim3(256), (size_t)n * CH * 3, ST(stream), scene, T, H, W, chunk_ids, frame_ids, n, dst);
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
    return gather_at<false, false>(scene, nullptr, 0, T, H, W, origins, frame_ids, nullptr, B, n, dst, dtype, stream);
}

extern "C" int ssr_scene_gather_bands(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W,
                                      const int32_t* origins, const int32_t* frame_ids, int32_t B, int32_t n, ssr_view dst,
                                      int32_t dtype, void* stream) {
    if (!bands || K <= 0) return SSR_EINVAL;
    return gather_at<true, false>(tci, bands, K, T, H, W, origins, frame_ids, nullptr, B, n, dst, dtype, stream);
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
    return blend_add<false>(src, dtype, origins, nullptr, B, C, window, acc, Ho, Wo, nonfinite, stream);
}

extern "C" int ssr_scene_blend_finish(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, uint8_t* mosaic, int32_t Ho,
                                      int32_t Wo, void* stream) {
    return blend_finish(acc, Sy, Sx, C, 65535u, mosaic, Ho, Wo, stream);
}

extern "C" int ssr_scene_gather_tf(const uint8_t* tci, const uint8_t* bands, int32_t K, int32_t T, int32_t H, int32_t W,
                                   const int32_t* origins, const int32_t* frame_ids, const int32_t* tf, int32_t B, int32_t n,
                                   ssr_view dst, int32_t dtype, void* stream) {
    if (!tf || K < 0 || (K > 0 && !bands)) return SSR_EINVAL;
    return gather_at<true, true>(tci, bands, K, T, H, W, origins, frame_ids, tf, B, n, dst, dtype, stream);
}

extern "C" int ssr_scene_blend_add_tf(ssr_view src, int32_t dtype, const int32_t* origins, const int32_t* tf, int32_t B, int32_t C,
                                      const int32_t* window, uint32_t* acc, int32_t Ho, int32_t Wo, int32_t* nonfinite, void* stream) {
    if (!tf) return SSR_EINVAL;
    return blend_add<true>(src, dtype, origins, tf, B, C, window, acc, Ho, Wo, nonfinite, stream);
}

extern "C" int ssr_scene_blend_finish_scaled(const uint32_t* acc, const int32_t* Sy, const int32_t* Sx, int32_t C, int32_t scale,
                                             uint8_t* mosaic, int32_t Ho, int32_t Wo, void* stream) {
    if (scale < 1) return SSR_EINVAL;
    return blend_finish(acc, Sy, Sx, C, (uint32_t)scale, mosaic, Ho, Wo, stream);
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
