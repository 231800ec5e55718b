// One element of the clip + Adam update, shared by k_adam_update (elementwise.hip) and k_msgd_alpha_update (msgd.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace fsmg {

// One element of the update.  The kernel has two loops over it (grid-stride, and chunks drawn from a counter) that must give the same
// bits, so which products are fused is spelled out here instead of left to the compiler's contraction, which decides per loop:
//   gc = g * scale;  m <- fma(gc, 1 - b1, b1 * m);  v <- fma((1 - b2) * gc, gc, b2 * v);  p <- p - (alpha * m) / (sqrt(v) + eps)
// (the fusions the single grid-stride loop was compiled to before the second loop existed: same bits as then)
__device__ __forceinline__ void adam_element(float g, float& m, float& v, float& p, float scale, float alpha) {
#pragma clang fp contract(off)
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float gc = g * scale;
    const float m_old = b1 * m, v_old = b2 * v, u = (1.0f - b2) * gc;
    m = __builtin_fmaf(gc, 1.0f - b1, m_old);
    v = __builtin_fmaf(u, gc, v_old);
    const float num = alpha * m, den = sqrtf(v) + eps;
    p = p - num / den;
}

}  // namespace fsmg
