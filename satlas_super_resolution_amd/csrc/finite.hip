// Non-finite guards (NaN / +-Inf) on the device.  The fp16-split forward of SSR_F32H turns an activation beyond 65504 or a packed weight
// beyond 64 into NaN outputs; these keep such a step from reaching the parameters, with every decision taken on the device:
//
//   ssr_nonfinite_scan      flag <- 1 if any element of one or more fp32 ranges is NaN / +-Inf.  Streams HBM: 16-byte loads per lane
//                           in a grid-stride loop, a scalar head / tail where a range does not start / end on a 16-byte boundary,
//                           a wave vote, then one plain store of 1 per wave that found something (every writer writes the same
//                           value: the result is order-independent).  No grid barrier, no spin-wait.
//   ssr_adam_step_guarded   ssr_adam_step (the same code, csrc/adam.h) while *flag == 0; otherwise param, moments and step stay and
//                           only the EMA moves toward the unchanged parameters.  Its single-thread tail counts the step or the skip
//                           and clears the flag for the next scan.
// The test is a bit test on the exponent ((bits & 0x7f800000) == 0x7f800000), not isnan / isinf: no fast-math flag can fold it away.
#include "adam.h"

namespace {

constexpr uint32_t EXP_BITS = 0x7f800000u;
__device__ __forceinline__ uint32_t nonfinite(uint32_t b) { return (b & EXP_BITS) == EXP_BITS; }
__device__ __forceinline__ uint32_t nonfinite4(const u32x4& v) {
    return nonfinite(v.x) | nonfinite(v.y) | nonfinite(v.z) | nonfinite(v.w);
}

struct ScanRanges {
    const float* p[SSR_SCAN_MAX_RANGES];
    long n[SSR_SCAN_MAX_RANGES];
};

// grid: (slices of the longest range, one row per range)
__global__ __launch_bounds__(256) void nonfinite_scan_kernel(const ScanRanges r, int32_t* __restrict__ flag) {
    const float* p = r.p[blockIdx.y];
    const long n = r.n[blockIdx.y];
    const long lead = (long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);   // floats before the first 16-byte boundary
    const long head = lead < n ? lead : n;
    const long nv = (n - head) >> 2, tail = head + 4 * nv;                               // [tail, n): at most 3 floats
    const u32x4* v = reinterpret_cast<const u32x4*>(p + head);
    const uint32_t* s = reinterpret_cast<const uint32_t*>(p);
    const long stride = (long)gridDim.x * blockDim.x;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    for (; i + 3 * stride < nv; i += 4 * stride)          // four 16-byte loads in flight per lane
        bad |= nonfinite4(v[i]) | nonfinite4(v[i + stride]) | nonfinite4(v[i + 2 * stride]) | nonfinite4(v[i + 3 * stride]);
    for (; i < nv; i += stride) bad |= nonfinite4(v[i]);
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        const long t = threadIdx.x;
        if (t < head) bad |= nonfinite(s[t]);
        if (tail + t < n) bad |= nonfinite(s[tail + t]);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) flag[0] = 1;
}

__global__ __launch_bounds__(256) void adam_guarded_kernel(const ssr_adam_args a, const int32_t* __restrict__ flag) {
    if (flag[0] == 0) adam_update(a);
    else adam_ema_only(a);
}

// the tail of ssr_adam_step (bump_kernel) for the guarded step: count the applied step or the skip, clear the flag
__global__ void guard_tail_kernel(int32_t* step, int32_t* flag, int32_t* skipped) {
    if (flag[0] == 0) step[0] += 1;
    else skipped[0] += 1;
    flag[0] = 0;
}

inline int grid_for(long total, int per_block, int cap) {
    long g = (total + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" int ssr_nonfinite_scan(const float* const* srcs, const int64_t* ns, int32_t n_ranges, int32_t* flag, void* stream) {
    if (!srcs || !ns || !flag || n_ranges <= 0 || n_ranges > SSR_SCAN_MAX_RANGES) return SSR_EINVAL;
    ScanRanges r{};
    long longest = 0;
    for (int k = 0; k < n_ranges; ++k) {
        if (ns[k] < 0 || (ns[k] > 0 && !srcs[k]) || (reinterpret_cast<uintptr_t>(srcs[k]) & 3)) return SSR_EINVAL;
        r.p[k] = srcs[k];
        r.n[k] = ns[k];
        if (ns[k] > longest) longest = ns[k];
    }
    if (longest == 0) return SSR_OK;
    hipLaunchKernelGGL(nonfinite_scan_kernel, dim3(grid_for(longest / 4, 256 * 4, 2048), n_ranges), dim3(256), 0, ST(stream), r, flag);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

extern "C" int ssr_adam_step_guarded(const ssr_adam_args* a, int32_t* flag, int32_t* skipped, void* stream) {
    if (!a || !a->param || !a->grad || !a->exp_avg || !a->exp_avg_sq || !a->lr || !a->step || a->n <= 0 || !flag || !skipped)
        return SSR_EINVAL;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3(grid_for(a->n, 256 * 4, 2048)), dim3(256), 0, ST(stream), *a, flag);
    SSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(guard_tail_kernel, dim3(1), dim3(1), 0, ST(stream), a->step, flag, skipped);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}
