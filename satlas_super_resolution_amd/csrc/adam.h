// torch.optim.Adam (single-tensor math) + the BasicSR model_ema update over one flat fp32 arena: the grid-stride bodies that the
// plain launch (csrc/misc.hip, ssr_adam_step) and the guarded one (csrc/finite.hip, ssr_adam_step_guarded) share, so that a
// guarded step that is not skipped does the same arithmetic bit for bit.
#pragma once
#include "common.h"

__device__ __forceinline__ float adam_ema_blend(const ssr_adam_args& a, long e, float p) {
    return a.ema[e] * a.ema_decay + p * (1.f - a.ema_decay);
}

__device__ __forceinline__ void adam_update(const ssr_adam_args& a) {
    const int t = a.step[0] + 1;
    const float lr = a.lr[0];
    const float bc1 = 1.f - powf(a.beta1, (float)t);
    const float bc2 = 1.f - powf(a.beta2, (float)t);
    const float step_size = lr / bc1;
    const float bc2_sqrt = sqrtf(bc2);
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += (long)gridDim.x * blockDim.x) {
        const float g = a.grad[e] * a.grad_scale;
        float m = a.exp_avg[e], v = a.exp_avg_sq[e];
        m = m + (g - m) * (1.f - a.beta1);                 // exp_avg.lerp_(grad, 1 - beta1)
        v = v * a.beta2 + (1.f - a.beta2) * g * g;         // mul_(beta2).addcmul_(g, g, 1 - beta2)
        const float denom = sqrtf(v) / bc2_sqrt + a.eps;
        const float p = a.param[e] - step_size * (m / denom);
        a.exp_avg[e] = m;
        a.exp_avg_sq[e] = v;
        a.param[e] = p;
        if (a.ema) a.ema[e] = adam_ema_blend(a, e, p);
    }
}

// an update that is not applied: param and moments stay, model_ema still runs (as on an iteration where the optimizer does not step)
__device__ __forceinline__ void adam_ema_only(const ssr_adam_args& a) {
    if (!a.ema) return;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += (long)gridDim.x * blockDim.x)
        a.ema[e] = adam_ema_blend(a, e, a.param[e]);
}
