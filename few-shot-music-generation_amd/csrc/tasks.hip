// Per-artist MAML: the fold behind one artist's query pass.  One HBM-bound float4 grid-stride pass that takes the artist's
// gradient into the running mean, forms and folds the Meta-SGD rate gradient where the rates are on, and puts theta back for the next
// artist; one thread folds the tail scalars.  wave64, no atomics, no reductions.
#include <algorithm>
#include "fsmg_kernels.h"

namespace fsmg {
namespace {

// acc <- w * g (the first artist) / fma(w, g, acc) (every later one): one rounding each, whatever the compiler would contract
__device__ __forceinline__ float fold_first(float w, float g) {
#pragma clang fp contract(off)
    return w * g;
}
__device__ __forceinline__ float fold_next(float w, float g, float acc) { return __builtin_fmaf(w, g, acc); }
// k_msgd_alpha_grad's element: -(g * s), one rounding (the negation is exact)
__device__ __forceinline__ float rate_grad(float g, float s) {
#pragma clang fp contract(off)
    return -(g * s);
}

// first / last are kernel arguments: every branch on them is wave-uniform.
//   first && last (N == 1): G is left alone, GA = -(G * S), P = P_saved
//   first           : ACC = w * G,            GA = w * -(G * S)
//   middle          : ACC = fma(w, G, ACC),   GA = fma(w, -(G * S), GA)
//   last            : G   = fma(w, G, ACC),   GA as in the middle
// The tail (a.n .. a.n + 5 of g / acc) and task_loss are one thread's work.
__global__ __launch_bounds__(256) void k_task_fold(const TaskFoldArgs a) {
    const long long n4 = a.n >> 2;
    const bool first = a.first != 0, last = a.last != 0, fold = !(first && last), rates = a.s != nullptr;
    const float w = a.w;
    float4* const out = reinterpret_cast<float4*>(last ? a.g : a.acc);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        // every load of the element first
        const float4 ps = reinterpret_cast<const float4*>(a.p_saved)[i];
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), ac = g, sv = g, ga = g;
        if (fold || rates) g = reinterpret_cast<const float4*>(a.g)[i];
        if (!first) ac = reinterpret_cast<const float4*>(a.acc)[i];
        if (rates) {
            sv = reinterpret_cast<const float4*>(a.s)[i];
            if (!first) ga = reinterpret_cast<const float4*>(a.ga)[i];
        }
        if (fold) {
            float4 o;
            if (first) { o.x = fold_first(w, g.x); o.y = fold_first(w, g.y); o.z = fold_first(w, g.z); o.w = fold_first(w, g.w); }
            else { o.x = fold_next(w, g.x, ac.x); o.y = fold_next(w, g.y, ac.y); o.z = fold_next(w, g.z, ac.z); o.w = fold_next(w, g.w, ac.w); }
            out[i] = o;
        }
        if (rates) {
            float4 r, o;
            r.x = rate_grad(g.x, sv.x); r.y = rate_grad(g.y, sv.y); r.z = rate_grad(g.z, sv.z); r.w = rate_grad(g.w, sv.w);
            if (!fold) o = r;
            else if (first) { o.x = fold_first(w, r.x); o.y = fold_first(w, r.y); o.z = fold_first(w, r.z); o.w = fold_first(w, r.w); }
            else { o.x = fold_next(w, r.x, ga.x); o.y = fold_next(w, r.y, ga.y); o.z = fold_next(w, r.z, ga.z); o.w = fold_next(w, r.w, ga.w); }
            reinterpret_cast<float4*>(a.ga)[i] = o;
        }
        reinterpret_cast<float4*>(a.p)[i] = ps;
    }
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const float* gt = a.g + a.n;
    float t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) t[k] = gt[k];
    if (a.task_loss != nullptr) *a.task_loss = t[1];
    if (!fold) return;
    float* const at = a.acc + a.n;
    float* const ot = (last ? a.g : a.acc) + a.n;
    const float ww = fold_first(w, w);
    float o[6];
    if (first) {
        o[0] = fold_first(ww, t[0]); o[1] = fold_first(w, t[1]);
#pragma unroll
        for (int k = 2; k < 6; ++k) o[k] = t[k] != 0.0f ? 1.0f : 0.0f;
    } else {
        o[0] = fold_next(ww, t[0], at[0]); o[1] = fold_next(w, t[1], at[1]);
#pragma unroll
        for (int k = 2; k < 6; ++k) o[k] = (t[k] != 0.0f || at[k] != 0.0f) ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) ot[k] = o[k];
}

}  // namespace

hipError_t launch_task_fold(hipStream_t s, const TaskFoldArgs& a) {
    if (a.g == nullptr || a.p == nullptr || a.p_saved == nullptr || a.n <= 0 || (a.n & 3) != 0) return hipErrorInvalidValue;
    if (!(a.first && a.last) && a.acc == nullptr) return hipErrorInvalidValue;
    if ((a.s != nullptr) != (a.ga != nullptr)) return hipErrorInvalidValue;
    const long long n4 = a.n >> 2;
    const int blocks = (int)std::max<long long>(1, std::min<long long>((n4 + 255) / 256, 2048));
    hipLaunchKernelGGL(k_task_fold, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fsmg
