// cwn_act.h -- the five activations of the CWN_ACT_* codes (include/cwn_hip.h), written once for every kernel that applies
// one: the library's own functions, no fast intrinsics.  A kernel templated on the code calls activate<ACT>; one that
// takes the code as an argument calls activate_rt.  File-local names, as the per-file copies were: include and call.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/cwn_hip.h"

namespace {

// ReLU and the max fold, the one spelling for every kernel: a NaN operand gives NaN, as torch.relu and scatter amax do.
// fmaxf / fmax return the operand that is NOT NaN (v_max_f32), which turns a diverged value into 0.  In float32 the
// propagating maximum is one instruction as well (v_maximum3_f32); float64 has none, so its ReLU is the compare and select
// and its cwn_max is what the compiler expands the builtin to: v_max_f64, an unordered compare and two selects.
// (cwn_relu, not relu: kernels keep a flag of that name.)
__device__ __forceinline__ float cwn_relu(float z) { return __builtin_elementwise_maximum(z, 0.f); }
__device__ __forceinline__ double cwn_relu(double z) { return z < 0.0 ? 0.0 : z; }
// ... and its gradient, from the activation's argument (or its output) y: the gradient passes unless y <= 0, torch's
// threshold_backward, so where y is NaN the gradient that arrives is handed on and not replaced by 0.
__device__ __forceinline__ float cwn_relu_bwd(float y, float dy) { return y <= 0.f ? 0.f : dy; }
__device__ __forceinline__ double cwn_relu_bwd(double y, double dy) { return y <= 0.0 ? 0.0 : dy; }
__device__ __forceinline__ float cwn_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ double cwn_max(double a, double b) { return __builtin_elementwise_maximum(a, b); }

template <int ACT>
__device__ __forceinline__ float activate(float z) {
    if constexpr (ACT == CWN_ACT_RELU) return cwn_relu(z);
    else if constexpr (ACT == CWN_ACT_ELU) return z > 0.f ? z : expm1f(z);
    else if constexpr (ACT == CWN_ACT_TANH) return tanhf(z);
    else if constexpr (ACT == CWN_ACT_SIGMOID) return 1.0f / (1.0f + expf(-z));
    else return z;
}

template <int ACT>
__device__ __forceinline__ double activate(double v) {
    if constexpr (ACT == CWN_ACT_RELU) return cwn_relu(v);
    else if constexpr (ACT == CWN_ACT_ELU) return v > 0.0 ? v : expm1(v);
    else if constexpr (ACT == CWN_ACT_TANH) return tanh(v);
    else if constexpr (ACT == CWN_ACT_SIGMOID) return 1.0 / (1.0 + exp(-v));
    else return v;
}

template <class real>
__device__ __forceinline__ real activate_rt(real z, int act) {
    switch (act) {
        case CWN_ACT_RELU: return activate<CWN_ACT_RELU>(z);
        case CWN_ACT_ELU: return activate<CWN_ACT_ELU>(z);
        case CWN_ACT_TANH: return activate<CWN_ACT_TANH>(z);
        case CWN_ACT_SIGMOID: return activate<CWN_ACT_SIGMOID>(z);
        default: return z;
    }
}

// dy * act'(z) from the pre-activation z, by torch's backward formulas -- so a non-finite z or dy gives what torch gives:
//   id       dy
//   relu     dy unless z <= 0 (cwn_relu_bwd: a select, no product -- an infinite dy behind a closed gate is 0, not NaN)
//   elu      z > 0 ? dy : dy * exp(z)             (alpha = 1; written so that a NaN z gives NaN, as torch's elu_backward
//                                                  on the CPU does -- its blend keeps the exp branch unless z > 0)
//   tanh     dy * (1 - y * y)                     y = activate<ACT>(z): the forward's bits
//   sigmoid  dy * (y * (1 - y))
// One text for float and double; expf / exp are picked by overload.
__device__ __forceinline__ float cwn_exp(float z) { return expf(z); }
__device__ __forceinline__ double cwn_exp(double z) { return exp(z); }

template <int ACT, class real>
__device__ __forceinline__ real activate_bwd(real z, real dy) {
    if constexpr (ACT == CWN_ACT_RELU) return cwn_relu_bwd(z, dy);
    else if constexpr (ACT == CWN_ACT_ELU) return z > real(0.0) ? dy : dy * cwn_exp(z);
    else if constexpr (ACT == CWN_ACT_TANH) {
        const real y = activate<ACT>(z);
        return dy * (real(1.0) - y * y);
    } else if constexpr (ACT == CWN_ACT_SIGMOID) {
        const real y = activate<ACT>(z);
        return dy * (y * (real(1.0) - y));
    } else return dy;
}

// act'(z) as a function of out = act(z)
__device__ __forceinline__ float act_grad(int act, float o) {
    switch (act) {
        case CWN_ACT_RELU: return o > 0.f ? 1.f : 0.f;
        case CWN_ACT_ELU: return o > 0.f ? 1.f : o + 1.f;
        case CWN_ACT_TANH: return 1.f - o * o;
        case CWN_ACT_SIGMOID: return o * (1.f - o);
        default: return 1.f;
    }
}

// is `act` one of the CWN_ACT_* codes?  (host)
inline bool known_act(int act) { return act >= CWN_ACT_ID && act <= CWN_ACT_SIGMOID; }

}  // namespace
