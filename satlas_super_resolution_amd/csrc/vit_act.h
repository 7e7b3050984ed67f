// The activations of the vision towers (SSR_VIT_ACT_*), one definition for ssr_linear's fused epilogue (vit.hip) and for the separate
// activation pass of the training plan (vit_bwd.hip): the same expression on the same fp32 value gives the same bytes.
#pragma once
#include "common.h"
#include <math.h>

__device__ __forceinline__ float vit_act(float v, int act) {
    switch (act) {
        case SSR_VIT_ACT_QUICK_GELU: return v / (1.0f + expf(-1.702f * v));                         // x * sigmoid(1.702 x)
        case SSR_VIT_ACT_GELU_TANH: return 0.5f * v * (1.0f + tanhf(0.7978845608028654f * (v + 0.044715f * v * v * v)));
        case SSR_VIT_ACT_GELU_ERF: return 0.5f * v * (1.0f + erff(v * 0.7071067811865476f));
        default: return v;
    }
}
