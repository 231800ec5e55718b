// Meta-SGD: the inner step of the MAML-style pass with a learned rate per parameter element, the first-order gradient
// with respect to the rates, their clip + Adam + clamp.  HBM-bound float4 grid-stride passes; wave64, fixed-order fp64 reductions,
// no atomics.
#include <algorithm>
#include "fsmg_kernels.h"
#include "adam_element.h"

namespace fsmg {
namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// S <- fma(step, g, S): the applied support gradient of this inner step, one rounding, whatever the compiler would contract
__device__ __forceinline__ float sum_element(float step, float g, float s) {
#pragma clang fp contract(off)
    return __builtin_fmaf(step, g, s);
}
// st = step * alpha, rounded once on its own: the product below may fuse into its subtraction, this one must not fuse into anything
__device__ __forceinline__ float rate_element(float step, float alpha) {
#pragma clang fp contract(off)
    return step * alpha;
}

// k_sgd_update with a rate per element.  Every block re-derives the step from the same partials in the same order as k_sgd_update does
// and returns at once on the same conditions; the element line `p -= st * g` is k_sgd_update's source expression, so with alpha == 1
// (st == step exactly) the two kernels write the same bits.
template <bool WITH_SUM>
__global__ __launch_bounds__(256) void k_msgd_update(const MsgdUpdateArgs a) {
    __shared__ double sh[4];
    __shared__ float s_scale;
    if ((a.err_flag != nullptr && *a.err_flag != 0) || a.tail[2] != 0.0f || a.tail[3] != 0.0f || a.tail[4] != 0.0f || a.tail[5] != 0.0f) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int i = tid; i < a.n_partials; i += 256) s += a.partials[i];
    s = wave_sum_d(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double sq = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (a.use_slices) sq += (double)a.tail[0];
        const double gnorm = sqrt(sq), clip = (double)a.clip;
        s_scale = (float)(clip / fmax(gnorm, clip)) * a.lr;
        if (a.gnorm_out != nullptr && blockIdx.x == 0) *a.gnorm_out = (float)gnorm;
    }
    __syncthreads();
    const float step = s_scale;
    const long long n4 = a.n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 g = reinterpret_cast<const float4*>(a.g)[i];
        const float4 r = reinterpret_cast<const float4*>(a.alpha)[i];
        float4 p = reinterpret_cast<float4*>(a.p)[i];
        float4 st;
        st.x = rate_element(step, r.x); st.y = rate_element(step, r.y); st.z = rate_element(step, r.z); st.w = rate_element(step, r.w);
        p.x -= st.x * g.x; p.y -= st.y * g.y; p.z -= st.z * g.z; p.w -= st.w * g.w;
        reinterpret_cast<float4*>(a.p)[i] = p;
        if (WITH_SUM) {
            float4 q = reinterpret_cast<float4*>(a.sum)[i];
            q.x = sum_element(step, g.x, q.x); q.y = sum_element(step, g.y, q.y); q.z = sum_element(step, g.z, q.z); q.w = sum_element(step, g.w, q.w);
            reinterpret_cast<float4*>(a.sum)[i] = q;
        }
    }
}

// GA = -(G * S): one rounding per element (the negation is exact)
__global__ __launch_bounds__(256) void k_msgd_alpha_grad(float* __restrict__ ga, const float* __restrict__ g, const float* __restrict__ sum, long long n4) {
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 x = reinterpret_cast<const float4*>(g)[i];
        const float4 y = reinterpret_cast<const float4*>(sum)[i];
        float4 o;
        o.x = -(x.x * y.x); o.y = -(x.y * y.y); o.z = -(x.z * y.z); o.w = -(x.w * y.w);
        reinterpret_cast<float4*>(ga)[i] = o;
    }
}

// clip + Adam + clamp of the rates.  The skip condition and the schedule are k_adam_update's; the norm is the plain global norm of GA
// from partials of its own.  Every block sums the partials in the same order, so the clip scale is the same on every block.
__global__ __launch_bounds__(256) void k_msgd_alpha_update(const MsgdAlphaArgs a) {
    __shared__ double sh[4];
    __shared__ float s_scale, s_alpha;
    if ((a.err_flag != nullptr && *a.err_flag != 0) || a.tail[2] != 0.0f || a.tail[3] != 0.0f || a.tail[4] != 0.0f || a.tail[5] != 0.0f) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int i = tid; i < a.n_partials; i += 256) s += a.partials[i];
    s = wave_sum_d(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const double gnorm = sqrt((sh[0] + sh[1]) + (sh[2] + sh[3])) * (double)a.grad_scale;
        const double clip = (double)a.clip;
        s_scale = a.clip > 0.0f ? (float)(clip / fmax(gnorm, clip) * (double)a.grad_scale) : a.grad_scale;
        const long long step = *a.step;
        const double t = (double)(step + 1);
        const double lr_s = (double)a.lr * pow(0.5, (double)step / (double)a.n_decay);
        s_alpha = (float)(lr_s * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
    }
    __syncthreads();
    const float scale = s_scale, alpha = s_alpha, lo = a.lo, hi = a.hi;
    const long long n4 = a.n >> 2;
#define FSMG_MSGD1(c) adam_element(g.c, m.c, v.c, p.c, scale, alpha); p.c = fminf(fmaxf(p.c, lo), hi);
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 g = reinterpret_cast<const float4*>(a.ga)[i];
        float4 m = reinterpret_cast<float4*>(a.m)[i];
        float4 v = reinterpret_cast<float4*>(a.v)[i];
        float4 p = reinterpret_cast<float4*>(a.alpha)[i];
        FSMG_MSGD1(x) FSMG_MSGD1(y) FSMG_MSGD1(z) FSMG_MSGD1(w)
        reinterpret_cast<float4*>(a.m)[i] = m;
        reinterpret_cast<float4*>(a.v)[i] = v;
        reinterpret_cast<float4*>(a.alpha)[i] = p;
    }
#undef FSMG_MSGD1
}

inline int pass_blocks(long long n4) { return (int)std::max<long long>(1, std::min<long long>((n4 + 255) / 256, 2048)); }

}  // namespace

hipError_t launch_msgd_update(hipStream_t s, const MsgdUpdateArgs& a) {
    if (a.p == nullptr || a.g == nullptr || a.alpha == nullptr || a.tail == nullptr || a.partials == nullptr || a.n <= 0 || (a.n & 3) != 0)
        return hipErrorInvalidValue;
    const int blocks = pass_blocks(a.n >> 2);
    if (a.sum != nullptr) hipLaunchKernelGGL(k_msgd_update<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_msgd_update<false>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_msgd_alpha_grad(hipStream_t s, float* ga, const float* g, const float* sum, long long n) {
    if (ga == nullptr || g == nullptr || sum == nullptr || n <= 0 || (n & 3) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_msgd_alpha_grad, dim3(pass_blocks(n >> 2)), dim3(256), 0, s, ga, g, sum, n >> 2);
    return hipGetLastError();
}

hipError_t launch_msgd_alpha_update(hipStream_t s, const MsgdAlphaArgs& a) {
    if (a.alpha == nullptr || a.m == nullptr || a.v == nullptr || a.ga == nullptr || a.partials == nullptr || a.tail == nullptr || a.step == nullptr ||
        a.n <= 0 || (a.n & 3) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_msgd_alpha_update, dim3(pass_blocks(a.n >> 2)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fsmg
