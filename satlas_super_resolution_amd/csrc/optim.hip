// BasicSR's other optimizers (get_optimizer: Adam with weight decay / amsgrad, AdamW, SGD, RMSprop) + the model_ema update over one flat
// fp32 arena: ssr_optim_step and ssr_optim_step_guarded.  Each kind follows the single-tensor path of torch.optim (adam.py
// _single_tensor_adam, sgd.py _single_tensor_sgd, rmsprop.py _single_tensor_rmsprop), operation by operation, with what ssr_adam_step has:
// grad_scale folded into the gradient load, lr and step as device scalars, the EMA blend fused, one grid-stride coalesced loop.
//
//   * kind Adam with weight_decay 0 and no amsgrad IS ssr_adam_step / ssr_adam_step_guarded (csrc/adam.h): the call is forwarded, so
//     that arithmetic has one definition and the two entry points agree bit for bit.
//   * the guarded launch reads *flag on the device: 0 -> the update; otherwise parameters, every state arena and *step stay, the EMA
//     still moves toward the unchanged parameters.  The single-thread tail counts the step or the skip and clears the flag.
//   * SGD's first applied step sets momentum_buffer = g (torch: the buffer does not exist yet), every later one
//     buf = momentum buf + (1 - dampening) g: decided by *step == 0, which a skipped step leaves as it is.
//   * centered RMSprop takes sqrt(square_avg - grad_avg^2) without a clamp, as torch does.
// State arenas that an option does not need are NULL and never touched.
#include "adam.h"

namespace {

__device__ __forceinline__ float optim_ema_blend(const ssr_optim_args& a, long e, float p) {
    return a.ema[e] * a.ema_decay + p * (1.f - a.ema_decay);
}

#define OPTIM_LOOP(e, a) for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (a).n; e += (long)gridDim.x * blockDim.x)

// Adam (weight decay coupled: g += wd p) and AdamW (decoupled: p *= 1 - lr wd), amsgrad optional
template <bool DECOUPLED>
__device__ __forceinline__ void adam_wd_update(const ssr_optim_args& a) {
    const int t = a.step[0] + 1;
    const float lr = a.lr[0];
    const float bc1 = 1.f - powf(a.beta1, (float)t);
    const float bc2 = 1.f - powf(a.beta2, (float)t);
    const float step_size = lr / bc1;
    const float bc2_sqrt = sqrtf(bc2);
    const float wd = a.weight_decay;
    const float shrink = 1.f - lr * wd;                       // param.mul_(1 - lr * weight_decay)
    const bool ams = (a.flags & SSR_OPT_AMSGRAD) != 0;
    OPTIM_LOOP(e, a) {
        float g = a.grad[e] * a.grad_scale;
        float p = a.param[e];
        if (wd != 0.f) {
            if (DECOUPLED) p = p * shrink;
            else g = g + wd * p;                               // grad.add(param, alpha=weight_decay)
        }
        float m = a.exp_avg[e], v = a.exp_avg_sq[e];
        m = m + (g - m) * (1.f - a.beta1);                     // exp_avg.lerp_(grad, 1 - beta1)
        v = v * a.beta2 + (1.f - a.beta2) * g * g;             // mul_(beta2).addcmul_(g, g, 1 - beta2)
        float vd = v;
        if (ams) {                                             // torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
            vd = fmaxf(a.max_exp_avg_sq[e], v);
            a.max_exp_avg_sq[e] = vd;
        }
        const float denom = sqrtf(vd) / bc2_sqrt + a.eps;
        p = p - step_size * (m / denom);
        a.exp_avg[e] = m;
        a.exp_avg_sq[e] = v;
        a.param[e] = p;
        if (a.ema) a.ema[e] = optim_ema_blend(a, e, p);
    }
}

__device__ __forceinline__ void sgd_update(const ssr_optim_args& a) {
    const bool first = a.step[0] == 0;
    const float lr = a.lr[0];
    const float wd = a.weight_decay, mom = a.momentum;
    const float keep = 1.f - a.dampening;
    const bool nesterov = (a.flags & SSR_OPT_NESTEROV) != 0;
    OPTIM_LOOP(e, a) {
        float g = a.grad[e] * a.grad_scale;
        float p = a.param[e];
        if (wd != 0.f) g = g + wd * p;
        if (mom != 0.f) {
            float buf = g;                                     // buf = grad.clone() on the first step
            if (!first) buf = a.momentum_buffer[e] * mom + keep * g;      // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
            a.momentum_buffer[e] = buf;
            g = nesterov ? g + mom * buf : buf;
        }
        p = p - lr * g;                                        // param.add_(grad, alpha=-lr)
        a.param[e] = p;
        if (a.ema) a.ema[e] = optim_ema_blend(a, e, p);
    }
}

__device__ __forceinline__ void rmsprop_update(const ssr_optim_args& a) {
    const float lr = a.lr[0];
    const float wd = a.weight_decay, mom = a.momentum, alpha = a.alpha;
    const bool centered = (a.flags & SSR_OPT_CENTERED) != 0;
    OPTIM_LOOP(e, a) {
        float g = a.grad[e] * a.grad_scale;
        float p = a.param[e];
        if (wd != 0.f) g = g + wd * p;
        float sq = a.square_avg[e];
        sq = sq * alpha + (1.f - alpha) * g * g;               // square_avg.mul_(alpha).addcmul_(g, g, 1 - alpha)
        a.square_avg[e] = sq;
        float avg;
        if (centered) {
            float ga = a.grad_avg[e];
            ga = ga + (g - ga) * (1.f - alpha);                // grad_avg.lerp_(grad, 1 - alpha)
            a.grad_avg[e] = ga;
            avg = sqrtf(sq - ga * ga);                         // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_(): no clamp
        } else {
            avg = sqrtf(sq);
        }
        avg = avg + a.eps;
        if (mom > 0.f) {
            const float buf = a.momentum_buffer[e] * mom + g / avg;       // buf.mul_(momentum).addcdiv_(grad, avg)
            a.momentum_buffer[e] = buf;
            p = p - lr * buf;
        } else {
            p = p - lr * (g / avg);                            // param.addcdiv_(grad, avg, value=-lr)
        }
        a.param[e] = p;
        if (a.ema) a.ema[e] = optim_ema_blend(a, e, p);
    }
}

// an update that is not applied: param and every state arena stay, model_ema still runs
__device__ __forceinline__ void optim_ema_only(const ssr_optim_args& a) {
    if (!a.ema) return;
    OPTIM_LOOP(e, a) a.ema[e] = optim_ema_blend(a, e, a.param[e]);
}

template <int KIND>
__device__ __forceinline__ void optim_update(const ssr_optim_args& a) {
    if (KIND == SSR_OPT_ADAM) adam_wd_update<false>(a);
    else if (KIND == SSR_OPT_ADAMW) adam_wd_update<true>(a);
    else if (KIND == SSR_OPT_SGD) sgd_update(a);
    else rmsprop_update(a);
}

// flag == NULL: the plain launch
template <int KIND>
__global__ __launch_bounds__(256) void optim_kernel(const ssr_optim_args a, const int32_t* __restrict__ flag) {
    if (!flag || flag[0] == 0) optim_update<KIND>(a);
    else optim_ema_only(a);
}

// count the applied step or the skip, clear the flag (one thread, behind the update on the same stream)
__global__ void optim_tail_kernel(int32_t* step, int32_t* flag, int32_t* skipped) {
    if (!flag) { step[0] += 1; return; }
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

// SSR_OK, or why the arguments cannot be launched
int optim_validate(const ssr_optim_args* a) {
    if (!a || !a->param || !a->grad || !a->lr || !a->step || a->n <= 0) return SSR_EINVAL;
    const bool ams = a->flags & SSR_OPT_AMSGRAD, nest = a->flags & SSR_OPT_NESTEROV, cen = a->flags & SSR_OPT_CENTERED;
    switch (a->kind) {
    case SSR_OPT_ADAM:
    case SSR_OPT_ADAMW:
        if (!a->exp_avg || !a->exp_avg_sq || (ams && !a->max_exp_avg_sq) || nest || cen) return SSR_EINVAL;
        return SSR_OK;
    case SSR_OPT_SGD:
        if (ams || cen || !(a->momentum >= 0.f) || (a->momentum != 0.f && !a->momentum_buffer)) return SSR_EINVAL;
        if (nest && (a->momentum <= 0.f || a->dampening != 0.f)) return SSR_EINVAL;      // torch: "Nesterov momentum requires a momentum and zero dampening"
        return SSR_OK;
    case SSR_OPT_RMSPROP:
        if (ams || nest || !a->square_avg || (cen && !a->grad_avg) || !(a->momentum >= 0.f) || (a->momentum > 0.f && !a->momentum_buffer))
            return SSR_EINVAL;
        return SSR_OK;
    default:
        return SSR_EUNSUP;
    }
}

inline bool is_plain_adam(const ssr_optim_args* a) {
    return a->kind == SSR_OPT_ADAM && a->weight_decay == 0.f && !(a->flags & SSR_OPT_AMSGRAD);
}

inline ssr_adam_args as_adam(const ssr_optim_args* a) {
    ssr_adam_args r;
    r.param = a->param; r.grad = a->grad; r.exp_avg = a->exp_avg; r.exp_avg_sq = a->exp_avg_sq; r.ema = a->ema; r.n = a->n;
    r.lr = a->lr; r.step = a->step; r.beta1 = a->beta1; r.beta2 = a->beta2; r.eps = a->eps; r.ema_decay = a->ema_decay;
    r.grad_scale = a->grad_scale;
    return r;
}

#define ST(s) reinterpret_cast<hipStream_t>(s)

int optim_launch(const ssr_optim_args* a, int32_t* flag, int32_t* skipped, void* stream) {
    const dim3 grid(grid_for(a->n, 256 * 4, 2048)), block(256);
    switch (a->kind) {
    case SSR_OPT_ADAM: hipLaunchKernelGGL(optim_kernel<SSR_OPT_ADAM>, grid, block, 0, ST(stream), *a, flag); break;
    case SSR_OPT_ADAMW: hipLaunchKernelGGL(optim_kernel<SSR_OPT_ADAMW>, grid, block, 0, ST(stream), *a, flag); break;
    case SSR_OPT_SGD: hipLaunchKernelGGL(optim_kernel<SSR_OPT_SGD>, grid, block, 0, ST(stream), *a, flag); break;
    default: hipLaunchKernelGGL(optim_kernel<SSR_OPT_RMSPROP>, grid, block, 0, ST(stream), *a, flag); break;
    }
    SSR_LAUNCH_CHECK();
    hipLaunchKernelGGL(optim_tail_kernel, dim3(1), dim3(1), 0, ST(stream), a->step, flag, skipped);
    SSR_LAUNCH_CHECK();
    return SSR_OK;
}

}  // namespace

extern "C" int ssr_optim_step(const ssr_optim_args* a, void* stream) {
    const int rc = optim_validate(a);
    if (rc != SSR_OK) return rc;
    if (is_plain_adam(a)) {
        const ssr_adam_args r = as_adam(a);
        return ssr_adam_step(&r, stream);
    }
    return optim_launch(a, nullptr, nullptr, stream);
}

extern "C" int ssr_optim_step_guarded(const ssr_optim_args* a, int32_t* flag, int32_t* skipped, void* stream) {
    const int rc = optim_validate(a);
    if (rc != SSR_OK) return rc;
    if (!flag || !skipped) return SSR_EINVAL;
    if (is_plain_adam(a)) {
        const ssr_adam_args r = as_adam(a);
        return ssr_adam_step_guarded(&r, flag, skipped, stream);
    }
    return optim_launch(a, flag, skipped, stream);
}
