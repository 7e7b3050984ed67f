// Batched PNG decode on the device for whole-tile inference (`png_decode: device` of infer_grid, satlas_super_resolution_amd/
// png_device.py): the 64-256 input stacks of a batch are inflated and unfiltered side by side and stay on the device; the zero test
// and the frame pick of select_frames / format_s2naip_data run on the decoded stacks where they lie.
//
//   ssr_png_decode        n zlib streams (the concatenated IDAT payloads of n PNG files) -> tight [H][W][C] bytes, status per item
//   ssr_png_decode_host   the same core (csrc/png_inflate.h) on the CPU, host pointers: the twin the CPU tests and the sanitizer
//                         program run
//   ssr_stack_zero_scan   per (stack, frame): does the 32 x 32 x 3 frame hold a zero sample
//   ssr_stack_gather      the chosen frames of every stack -> uint8 [B][n][32][32][3], frame 0 of every stack -> [B][32][32][3]
//
// png_decode_kernel: one wave (a block of 64 threads) per item.  A DEFLATE stream is serial - every code's position depends on
// the lengths of all codes before it - so the wave walks it in lockstep, all lanes computing the same bit reader state from the
// same bytes (LDS broadcasts), and spreads what is parallel over its lanes: match copies, stored blocks, the None / Up scanlines
// and the Adler sums.  The parallelism that fills the chip is across the items of a batch.
//   LDS per block: the code tables (pngi_work, 3 KiB) and a pool the caller sizes (lds_pool).  An item's compressed stream is
//   staged into the pool when it fits (our chunks: 10-40 KB), and its raw scanlines (the inflate output = the history window)
//   live in the rest of the pool when they fit there; what does not fit is read from / written to global memory (the stream in
//   place, the scanlines in the caller's scratch at raw_off).  The core sees plain pointers either way.
//   Nothing is shared between blocks and nothing is accumulated: two launches on the same input give the same bytes.
#include "common.h"
#include "png_inflate.h"

namespace {

#define ST(s) reinterpret_cast<hipStream_t>(s)

constexpr int WORK_BYTES = (int)((sizeof(pngi_work) + 15) / 16 * 16);
constexpr int LDS_MAX = 160 * 1024;
constexpr int FRAME = 32 * 32 * 3;      // bytes of one frame of a stack
constexpr int FRAME16 = FRAME / 16;

static_assert(sizeof(ssr_png_item) == 40, "ssr_png_item layout (include/ssr_hip.h, hip.PngItem)");

inline int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

__global__ __launch_bounds__(64) void png_decode_kernel(const uint8_t* __restrict__ streams, int64_t streams_len,
                                                        const ssr_png_item* __restrict__ items, uint8_t* dst, int64_t dst_len,
                                                        uint8_t* scratch, int64_t scratch_len, int32_t* __restrict__ status,
                                                        int32_t lds_pool) {
    extern __shared__ uint4 png_lds[];
    const int lane = threadIdx.x;
    const ssr_png_item it = items[blockIdx.x];
    if (!pngi_item_ok(it.src_off, it.src_len, it.width, it.height, it.channels, it.dst_off, it.raw_off, streams_len, dst_len,
                      scratch_len)) {                                   // block-uniform
        if (lane == 0) status[blockIdx.x] = PNGI_EDESC;
        return;
    }
    pngi_work* wk = reinterpret_cast<pngi_work*>(png_lds);
    uint8_t* pool = reinterpret_cast<uint8_t*>(png_lds) + WORK_BYTES;
    const uint8_t* src = streams + it.src_off;
    const int64_t raw_len = (int64_t)it.height * ((int64_t)it.width * it.channels + 1);
    int64_t used = 0;
    if (((int64_t)it.src_len + 15) / 16 * 16 <= lds_pool) {              // the stream into LDS
        const int n = it.src_len;
        if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            uint32_t* d4 = reinterpret_cast<uint32_t*>(pool);
            for (int i = lane; i < n / 4; i += 64) d4[i] = s4[i];
            for (int i = (n & ~3) + lane; i < n; i += 64) pool[i] = src[i];
        } else {
            for (int i = lane; i < n; i += 64) pool[i] = src[i];
        }
        src = pool;
        used = ((int64_t)n + 15) / 16 * 16;
    }
    uint8_t* raw = raw_len <= lds_pool - used ? pool + used : scratch + it.raw_off;
    __syncthreads();
    const int st = pngi_decode_image(src, (uint32_t)it.src_len, (uint32_t)it.width, (uint32_t)it.height, (uint32_t)it.channels, raw,
                                     dst + it.dst_off, wk, lane, 64);
    if (lane == 0) status[blockIdx.x] = st;
}

__device__ __forceinline__ bool zero_byte_in(uint32_t v) { return ((v - 0x01010101u) & ~v & 0x80808080u) != 0; }

// one wave per (stack, frame): 192 uint4 = 3 per lane when the frame is 16-byte aligned, single bytes otherwise
__global__ __launch_bounds__(256) void stack_zero_scan_kernel(const uint8_t* __restrict__ buf, int64_t buf_len,
                                                              const int64_t* __restrict__ offs, const int32_t* __restrict__ Ts, int B,
                                                              int Tmax, uint8_t* __restrict__ has_zero) {
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (long)B * Tmax) return;                                 // wave-uniform
    const int lane = threadIdx.x & 63;
    const int b = (int)(item / Tmax), t = (int)(item - (long)b * Tmax);
    const int64_t off = offs[b];
    const int64_t T = Ts[b];
    bool z = false;
    if (t < T && T <= Tmax && off >= 0 && off <= buf_len && T * FRAME <= buf_len - off) {      // wave-uniform
        const uint8_t* f = buf + off + (int64_t)t * FRAME;
        if ((reinterpret_cast<uintptr_t>(f) & 15) == 0) {
#pragma unroll
            for (int k = 0; k < FRAME16 / 64; ++k) {
                const uint4 v = reinterpret_cast<const uint4*>(f)[lane + 64 * k];
                z |= zero_byte_in(v.x) | zero_byte_in(v.y) | zero_byte_in(v.z) | zero_byte_in(v.w);
            }
        } else {
            for (int i = lane; i < FRAME; i += 64) z |= f[i] == 0;
        }
    }
    const bool any = __any(z);
    if (lane == 0) has_zero[item] = any ? 1 : 0;
}

// one block per (stack, slot): slots 0 .. n - 1 are the chosen frames, slot n is frame 0 -> `first`
__global__ __launch_bounds__(256) void stack_gather_kernel(const uint8_t* __restrict__ buf, int64_t buf_len,
                                                           const int64_t* __restrict__ offs, const int32_t* __restrict__ Ts,
                                                           const int32_t* __restrict__ frame_ids, int n, uint8_t* __restrict__ out,
                                                           uint8_t* __restrict__ first) {
    const int b = blockIdx.x / (n + 1), k = blockIdx.x - b * (n + 1);
    const int64_t off = offs[b];
    const int64_t T = Ts[b];
    if (T < 1 || off < 0 || off > buf_len || T * FRAME > buf_len - off) return;     // block-uniform: a stack outside the buffer is a no-op
    const int64_t t = k < n ? frame_ids[(long)b * n + k] : 0;
    if (t < 0 || t >= T) return;
    const uint8_t* f = buf + off + t * FRAME;
    uint8_t* o = k < n ? out + ((long)b * n + k) * FRAME : first + (long)b * FRAME;
    if (((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(o)) & 15) == 0) {
        if (threadIdx.x < FRAME16) reinterpret_cast<uint4*>(o)[threadIdx.x] = reinterpret_cast<const uint4*>(f)[threadIdx.x];
    } else {
        for (int i = threadIdx.x; i < FRAME; i += 256) o[i] = f[i];
    }
}

int lds_optin(int lds) {
    static bool done[SSR_MAX_DEVICES];
    const int dev = ssr_device_ordinal();
    if (lds > 64 * 1024 && !done[dev]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(png_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           LDS_MAX);
        if (e != hipSuccess) return (int)e;
        done[dev] = true;
    }
    return SSR_OK;
}

}  // namespace

extern "C" int64_t ssr_png_scratch_bytes(int32_t width, int32_t height, int32_t channels) {
    if (width < 1 || height < 1 || width > 32768 || height > 32768 || (channels != 1 && channels != 3)) return -1;
    const int64_t raw = (int64_t)height * ((int64_t)width * channels + 1);
    return raw > (int64_t)PNGI_MAX_RAW ? -1 : align16(raw);
}

extern "C" int32_t ssr_png_lds_pool_max(void) { return LDS_MAX - WORK_BYTES; }

extern "C" int ssr_png_decode(const uint8_t* streams, int64_t streams_len, const ssr_png_item* items, int32_t n, uint8_t* dst,
                              int64_t dst_len, uint8_t* scratch, int64_t scratch_len, int32_t* status, int32_t lds_pool, void* stream) {
    if (!streams || !items || !dst || !scratch || !status || n <= 0 || streams_len < 0 || dst_len < 0 || scratch_len < 0 || lds_pool < 0)
        return SSR_EINVAL;
    if (n > (1 << 20) || lds_pool > LDS_MAX - WORK_BYTES) return SSR_EUNSUP;
    const int lds = WORK_BYTES + (lds_pool + 15) / 16 * 16;
    const int rc = lds_optin(lds);
    if (rc) return rc;
    hipLaunchKernelGGL(png_decode_kernel, dim3(n), dim3(64), lds, ST(stream), streams, streams_len, items, dst, dst_len, scratch,
                       scratch_len, status, lds_pool);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_png_decode_host(const uint8_t* streams, int64_t streams_len, const ssr_png_item* items, int32_t n, uint8_t* dst,
                                   int64_t dst_len, uint8_t* scratch, int64_t scratch_len, int32_t* status) {
    if (!streams || !items || !dst || !scratch || !status || n <= 0 || streams_len < 0 || dst_len < 0 || scratch_len < 0) return SSR_EINVAL;
    if (n > (1 << 20)) return SSR_EUNSUP;
    pngi_work wk;
    for (int i = 0; i < n; ++i) {
        const ssr_png_item& it = items[i];
        if (!pngi_item_ok(it.src_off, it.src_len, it.width, it.height, it.channels, it.dst_off, it.raw_off, streams_len, dst_len,
                          scratch_len)) {
            status[i] = PNGI_EDESC;
            continue;
        }
        status[i] = pngi_decode_image(streams + it.src_off, (uint32_t)it.src_len, (uint32_t)it.width, (uint32_t)it.height,
                                      (uint32_t)it.channels, scratch + it.raw_off, dst + it.dst_off, &wk, 0, 1);
    }
    return SSR_OK;
}

extern "C" int ssr_stack_zero_scan(const uint8_t* buf, int64_t buf_len, const int64_t* offs, const int32_t* T, int32_t B, int32_t Tmax,
                                   uint8_t* has_zero, void* stream) {
    if (!buf || !offs || !T || !has_zero || B <= 0 || Tmax <= 0 || buf_len < 0) return SSR_EINVAL;
    const long items = (long)B * Tmax;
    if (items > (1l << 30)) return SSR_EUNSUP;
    hipLaunchKernelGGL(stack_zero_scan_kernel, dim3((int)((items + 3) / 4)), dim3(256), 0, ST(stream), buf, buf_len, offs, T, B, Tmax,
                       has_zero);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_stack_gather(const uint8_t* buf, int64_t buf_len, const int64_t* offs, const int32_t* T, const int32_t* frame_ids,
                                int32_t B, int32_t n, uint8_t* out, uint8_t* first, void* stream) {
    if (!buf || !offs || !T || !frame_ids || !out || !first || B <= 0 || n <= 0 || buf_len < 0) return SSR_EINVAL;
    if ((long)B * (n + 1) > (1l << 30)) return SSR_EUNSUP;
    hipLaunchKernelGGL(stack_gather_kernel, dim3(B * (n + 1)), dim3(256), 0, ST(stream), buf, buf_len, offs, T, frame_ids, n, out, first);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
