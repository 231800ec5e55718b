// The element of the learned optimiser (include/fsmg.h "learned optimiser"), shared by k_lopt_update and k_lopt_backprop
// (lopt.hip).  The back-propagation replays the inner trajectory and must arrive at the forward's bits, so nothing here is left to the
// compiler's contraction: every function states its own mode, and the fused operations are written as fmaf.
#pragma once
#include <hip/hip_runtime.h>

namespace fsmg {

constexpr int LOPT_NPHI = 14;           // wF[6], bF, wI[6], bI
constexpr int LOPT_MAX_STEPS = 8;       // inner steps a train form may store
constexpr float LOPT_EXP_M10 = 4.5399929762484854e-05f;   // e^-10
constexpr float LOPT_EXP_P10 = 22026.465794806718f;       // e^10

struct LoptPhi { float wF[6], bF, wI[6], bI; };

__device__ __forceinline__ LoptPhi lopt_load_phi(const float* __restrict__ phi) {
    LoptPhi w;
#pragma unroll
    for (int k = 0; k < 6; ++k) { w.wF[k] = phi[k]; w.wI[k] = phi[7 + k]; }
    w.bF = phi[6]; w.bI = phi[13];
    return w;
}

// the paper's preprocessing: (log|x| / 10, sign x) where |x| >= e^-10, (-1, e^10 x) below
__device__ __forceinline__ void lopt_prep(float x, float& a1, float& a2) {
#pragma clang fp contract(off)
    const float ax = fabsf(x);
    if (ax >= LOPT_EXP_M10) { a1 = logf(ax) / 10.0f; a2 = copysignf(1.0f, x); }
    else { a1 = -1.0f; a2 = LOPT_EXP_P10 * x; }
}

// sigmoid(w . (a1, a2, c1, c2, theta, prev) + b): a chain of six fmaf from the bias, then 1 / (1 + exp(-z))
__device__ __forceinline__ float lopt_gate(const float w[6], float b, float a1, float a2, float c1, float c2, float theta, float prev) {
#pragma clang fp contract(off)
    float z = __builtin_fmaf(w[0], a1, b);
    z = __builtin_fmaf(w[1], a2, z);
    z = __builtin_fmaf(w[2], c1, z);
    z = __builtin_fmaf(w[3], c2, z);
    z = __builtin_fmaf(w[4], theta, z);
    z = __builtin_fmaf(w[5], prev, z);
    return 1.0f / (1.0f + expf(-z));
}

// q = f * theta and st = step * (gate_scale * i): each product rounded on its own, fused into nothing
__device__ __forceinline__ float lopt_keep(float f, float theta) {
#pragma clang fp contract(off)
    return f * theta;
}
__device__ __forceinline__ float lopt_rate(float step, float gate_scale, float i) {
#pragma clang fp contract(off)
    const float gi = gate_scale * i;
    return step * gi;
}
// k_sgd_update's source expression `p - step * g` with q for p and st for step, contracted as that kernel's is: one fma
__device__ __forceinline__ float lopt_apply(float q, float st, float g) {
#pragma clang fp contract(fast)
    return q - st * g;
}

// one inner step of one element: the gates from (g, L, theta, previous gates), then theta
__device__ __forceinline__ float lopt_step_element(const LoptPhi& w, float g, float a1, float a2, float c1, float c2, float theta, float& F, float& I,
                                                   float step, float gate_scale) {
    const float f = lopt_gate(w.wF, w.bF, a1, a2, c1, c2, theta, F);
    const float i = lopt_gate(w.wI, w.bI, a1, a2, c1, c2, theta, I);
    F = f; I = i;
    return lopt_apply(lopt_keep(f, theta), lopt_rate(step, gate_scale, i), g);
}

}  // namespace fsmg
