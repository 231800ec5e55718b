// Learned optimiser: the inner step of the MAML-style pass as a meta-learner LSTM cell per parameter element (Ravi &
// Larochelle 2017, first order), the back-propagation through the stored inner steps, the reduction and the update of the fourteen shared
// weights.  HBM-bound float4 grid-stride passes; wave64, fixed-order fp64 reductions, no atomics.
#include <algorithm>
#include "fsmg_kernels.h"
#include "adam_element.h"
#include "lopt_element.h"

namespace fsmg {
namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool lopt_skipped(const int* err_flag, const float* tail) {
    return (err_flag != nullptr && *err_flag != 0) || tail[2] != 0.0f || tail[3] != 0.0f || tail[4] != 0.0f || tail[5] != 0.0f;
}

// k_sgd_update with the learned rule per element.  Every block re-derives the step from the same partials in the same order as
// k_sgd_update does and returns at once on the same conditions.  STORE (the train forms): g_t goes to its slot of the store, and block 0
// leaves step_t and L_t beside it for k_lopt_backprop.
template <bool STORE>
__global__ __launch_bounds__(256) void k_lopt_update(const LoptUpdateArgs a) {
    __shared__ double sh[4];
    __shared__ float s_scale;
    if (lopt_skipped(a.err_flag, a.tail)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int i = tid; i < a.n_partials; i += 256) s += a.partials[i];
    s = wave_sum_d(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    const float loss = a.tail[1];
    if (tid == 0) {
        double sq = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        if (a.use_slices) sq += (double)a.tail[0];
        const double gnorm = sqrt(sq), clip = (double)a.clip;
        s_scale = (float)(clip / fmax(gnorm, clip)) * a.lr;
        if (a.gnorm_out != nullptr && blockIdx.x == 0) *a.gnorm_out = (float)gnorm;
        if (STORE && blockIdx.x == 0) { *a.sc_step = s_scale; *a.sc_loss = loss; }
    }
    __syncthreads();
    const float step = s_scale, gs = a.gate_scale;
    const LoptPhi w = lopt_load_phi(a.phi);
    float c1, c2;
    lopt_prep(loss, c1, c2);
    const long long n4 = a.n >> 2;
#define FSMG_LOPT1(c) { float a1, a2; lopt_prep(g.c, a1, a2); p.c = lopt_step_element(w, g.c, a1, a2, c1, c2, p.c, F.c, I.c, step, gs); }
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        const float4 g = reinterpret_cast<const float4*>(a.g)[i];
        float4 p = reinterpret_cast<float4*>(a.p)[i];
        float4 F = reinterpret_cast<float4*>(a.F)[i];
        float4 I = reinterpret_cast<float4*>(a.I)[i];
        FSMG_LOPT1(x) FSMG_LOPT1(y) FSMG_LOPT1(z) FSMG_LOPT1(w)
        reinterpret_cast<float4*>(a.p)[i] = p;
        reinterpret_cast<float4*>(a.F)[i] = F;
        reinterpret_cast<float4*>(a.I)[i] = I;
        if (STORE) reinterpret_cast<float4*>(a.store)[i] = g;
    }
#undef FSMG_LOPT1
}

// One element through all K steps: the forward trajectory again from theta_0 and the stored gradients (lopt_element.h: the forward's
// bits), then the walk back of include/fsmg.h.  Products of two floats are exact in fp64, so the fourteen sums round only where they add.
template <int K>
__device__ __forceinline__ void lopt_back_element(const LoptPhi& w, const float (&g)[K], const float (&step)[K], const float (&c1)[K], const float (&c2)[K],
                                                  float gs, float theta0, float& D, float& thetaK, double (&acc)[LOPT_NPHI]) {
#pragma clang fp contract(off)
    float f[K], in[K], th[K], a1[K], a2[K];
    float theta = theta0, F = 1.0f, I = 0.0f;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        lopt_prep(g[t], a1[t], a2[t]);
        th[t] = theta;
        theta = lopt_step_element(w, g[t], a1[t], a2[t], c1[t], c2[t], theta, F, I, step[t], gs);
        f[t] = F; in[t] = I;
    }
    thetaK = theta;
    float d = D, carryF = 0.0f, carryI = 0.0f;
#pragma unroll
    for (int t = K - 1; t >= 0; --t) {
        const float Fp = t > 0 ? f[t - 1] : 1.0f, Ip = t > 0 ? in[t - 1] : 0.0f;
        const float dF = __builtin_fmaf(d, th[t], carryF);
        const float m = step[t] * gs;
        const float mg = m * g[t];
        const float dI = __builtin_fmaf(-d, mg, carryI);
        const float fd = f[t] * (1.0f - f[t]), id = in[t] * (1.0f - in[t]);
        const float pf = dF * fd, pi = dI * id;
        const double pfd = (double)pf, pid = (double)pi;
        acc[0] += pfd * (double)a1[t]; acc[1] += pfd * (double)a2[t]; acc[2] += pfd * (double)c1[t]; acc[3] += pfd * (double)c2[t];
        acc[4] += pfd * (double)th[t]; acc[5] += pfd * (double)Fp; acc[6] += pfd;
        acc[7] += pid * (double)a1[t]; acc[8] += pid * (double)a2[t]; acc[9] += pid * (double)c1[t]; acc[10] += pid * (double)c2[t];
        acc[11] += pid * (double)th[t]; acc[12] += pid * (double)Ip; acc[13] += pid;
        const float through = __builtin_fmaf(pf, w.wF[4], pi * w.wI[4]);
        d = __builtin_fmaf(d, f[t], through);
        carryF = pf * w.wF[5];
        carryI = pi * w.wI[5];
    }
    D = d;
}

// One launch for all K stored steps.  G is rewritten in place with the gradient through the learned rule; every block leaves its
// fourteen sums in part[block][14].  Returns at once where the update kernels skip.
template <int K>
__global__ __launch_bounds__(256) void k_lopt_backprop(const LoptBackpropArgs a) {
    __shared__ double sh[4][LOPT_NPHI];
    if (lopt_skipped(a.err_flag, a.tail)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LoptPhi w = lopt_load_phi(a.phi);
    const float gs = a.gate_scale;
    float step[K], c1[K], c2[K];
#pragma unroll
    for (int t = 0; t < K; ++t) { step[t] = a.sc[t]; lopt_prep(a.sc[LOPT_MAX_STEPS + t], c1[t], c2[t]); }
    double acc[LOPT_NPHI];
#pragma unroll
    for (int c = 0; c < LOPT_NPHI; ++c) acc[c] = 0.0;
    const long long n4 = a.n >> 2, stride4 = a.stride >> 2;
#define FSMG_LOPTB(c) { float gc[K]; _Pragma("unroll") for (int t = 0; t < K; ++t) gc[t] = g[t].c; \
                        lopt_back_element<K>(w, gc, step, c1, c2, gs, p.c, D.c, thK.c, acc); }
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n4; i += (long long)gridDim.x * 256) {
        float4 g[K];
#pragma unroll
        for (int t = 0; t < K; ++t) g[t] = reinterpret_cast<const float4*>(a.store)[(long long)t * stride4 + i];
        const float4 p = reinterpret_cast<const float4*>(a.p0)[i];
        float4 D = reinterpret_cast<float4*>(a.G)[i];
        float4 thK;
        FSMG_LOPTB(x) FSMG_LOPTB(y) FSMG_LOPTB(z) FSMG_LOPTB(w)
        reinterpret_cast<float4*>(a.G)[i] = D;
        if (a.theta_out != nullptr) reinterpret_cast<float4*>(a.theta_out)[i] = thK;
    }
#undef FSMG_LOPTB
#pragma unroll
    for (int c = 0; c < LOPT_NPHI; ++c) {
        const double v = wave_sum_d(acc[c]);
        if (lane == 0) sh[wave][c] = v;
    }
    __syncthreads();
    if (tid < LOPT_NPHI) a.part[(long long)blockIdx.x * LOPT_NPHI + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// One block.  reduce: the block partials in fixed order into the fp64 fold and GPhi = (float)fold -- fold = weight * sum where `first`,
// fold += weight * sum otherwise (the per-artist forms).  Otherwise the update inside apply_update: the plain global norm of GPhi, the
// optional clip, Adam on theta's schedule with phi_lr; skipped where k_adam_update skips.
__global__ __launch_bounds__(256) void k_lopt_phi(const LoptPhiArgs a) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (a.reduce) {
        for (int c = 0; c < LOPT_NPHI; ++c) {
            double s = 0.0;
            for (int i = tid; i < a.n_blocks; i += 256) s += a.part[(long long)i * LOPT_NPHI + c];
            s = wave_sum_d(s);
            if (lane == 0) sh[wave] = s;
            __syncthreads();
            if (tid == 0) {
                const double sum = ((sh[0] + sh[1]) + (sh[2] + sh[3])) * a.weight;
                const double v = a.first ? sum : a.fold[c] + sum;
                a.fold[c] = v;
                a.gphi[c] = (float)v;
            }
            __syncthreads();
        }
        return;
    }
    if (lopt_skipped(a.err_flag, a.tail)) return;
    __shared__ float s_scale, s_alpha;
    if (tid == 0) {
        double sq = 0.0;
        for (int c = 0; c < LOPT_NPHI; ++c) sq += (double)a.gphi[c] * (double)a.gphi[c];
        const double gnorm = sqrt(sq) * (double)a.grad_scale, clip = (double)a.clip;
        s_scale = a.clip > 0.0f ? (float)(clip / fmax(gnorm, clip) * (double)a.grad_scale) : a.grad_scale;
        const long long step = *a.step;
        const double t = (double)(step + 1);
        const double lr_s = (double)a.lr * pow(0.5, (double)step / (double)a.n_decay);
        s_alpha = (float)(lr_s * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
    }
    __syncthreads();
    if (tid < LOPT_NPHI) {
        float m = a.m[tid], v = a.v[tid], p = a.phi[tid];
        adam_element(a.gphi[tid], m, v, p, s_scale, s_alpha);
        a.m[tid] = m; a.v[tid] = v; a.phi[tid] = p;
    }
}

inline int pass_blocks(long long n4) { return (int)std::max<long long>(1, std::min<long long>((n4 + 255) / 256, LOPT_MAX_BLOCKS)); }

template <int K>
void launch_backprop_k(hipStream_t s, int blocks, const LoptBackpropArgs& a) {
    hipLaunchKernelGGL(k_lopt_backprop<K>, dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

int lopt_blocks(long long n) { return pass_blocks(n >> 2); }

hipError_t launch_lopt_update(hipStream_t s, const LoptUpdateArgs& a) {
    if (a.p == nullptr || a.g == nullptr || a.F == nullptr || a.I == nullptr || a.phi == nullptr || a.tail == nullptr || a.partials == nullptr ||
        a.n <= 0 || (a.n & 3) != 0 || (a.store != nullptr && (a.sc_step == nullptr || a.sc_loss == nullptr)))
        return hipErrorInvalidValue;
    const int blocks = pass_blocks(a.n >> 2);
    if (a.store != nullptr) hipLaunchKernelGGL(k_lopt_update<true>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_lopt_update<false>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lopt_backprop(hipStream_t s, const LoptBackpropArgs& a) {
    if (a.G == nullptr || a.p0 == nullptr || a.store == nullptr || a.sc == nullptr || a.phi == nullptr || a.part == nullptr || a.tail == nullptr ||
        a.n <= 0 || (a.n & 3) != 0 || a.stride < a.n || (a.stride & 3) != 0 || a.K < 1 || a.K > LOPT_MAX_STEPS)
        return hipErrorInvalidValue;
    const int blocks = pass_blocks(a.n >> 2);
    switch (a.K) {
        case 1: launch_backprop_k<1>(s, blocks, a); break;
        case 2: launch_backprop_k<2>(s, blocks, a); break;
        case 3: launch_backprop_k<3>(s, blocks, a); break;
        case 4: launch_backprop_k<4>(s, blocks, a); break;
        case 5: launch_backprop_k<5>(s, blocks, a); break;
        case 6: launch_backprop_k<6>(s, blocks, a); break;
        case 7: launch_backprop_k<7>(s, blocks, a); break;
        default: launch_backprop_k<8>(s, blocks, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_lopt_phi(hipStream_t s, const LoptPhiArgs& a) {
    if (a.gphi == nullptr) return hipErrorInvalidValue;
    if (a.reduce) {
        if (a.fold == nullptr || a.n_blocks < 0 || a.n_blocks > LOPT_MAX_BLOCKS || (a.n_blocks > 0 && a.part == nullptr)) return hipErrorInvalidValue;
    } else if (a.phi == nullptr || a.m == nullptr || a.v == nullptr || a.tail == nullptr || a.step == nullptr) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_lopt_phi, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fsmg
