// Dynamic evaluation: the window weights of a masked pass, the fused decay-to-theta update, the gradient statistics
// and the scatter of a window's scores.  HBM-bound float4 passes and small kernels; wave64, fixed-order fp64 reductions, no atomics
// on floating point.
#include <algorithm>
#include "fsmg_kernels.h"

namespace fsmg {
namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int clamp_len(int l, int T) { return min(max(l, 1), T); }

constexpr int DYN_CHUNK = 256 * 16;      // elements per partial (the thread -> element map of the squared-norm partials)

// win[0] = lo, win[1] = hi: the window the NEXT window pass reads (a captured pass replays with whatever stands there)
__global__ void k_set_window(int* __restrict__ win, int lo, int hi) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { win[0] = lo; win[1] = hi; }
}

// k_row_weights with a window [lo, hi) read from win[0..1]; one group of B rows.  e[b] = min(hi, len[b]):
//   n_valid = sum_b max(0, e[b] - lo)  (integers: exact, whatever the order)
//   w[t * B + b] = lo <= t < e[b] ? (float)(1 / ((double)n_valid + 1e-12)) : 0
//   elen[b] = e[b]: what the token prep of the pass takes as the row's length (fixed ids from there on)
// A length outside [1, T] raises the token-range flag and is clamped.  Block y: every block sums the lengths itself, block 0 publishes.
__global__ __launch_bounds__(256) void k_window_weights(const int* __restrict__ len, int B, int T, const int* __restrict__ win,
                                                        float* __restrict__ w, int* __restrict__ n_valid, int* __restrict__ elen,
                                                        int* __restrict__ err_flag) {
    __shared__ int s_sum;
    const int tid = threadIdx.x;
    const int lo = min(max(win[0], 0), T), hi = min(max(win[1], lo), T);
    if (tid == 0) s_sum = 0;
    __syncthreads();
    int mine = 0;
    bool bad = false;
    for (int b = tid; b < B; b += 256) {
        const int l = len[b];
        if (l < 1 || l > T) bad = true;
        const int e = min(hi, clamp_len(l, T));
        mine += max(0, e - lo);
        if (blockIdx.x == 0) elen[b] = max(e, 1);
    }
    if (mine) atomicAdd(&s_sum, mine);
    if (bad && blockIdx.x == 0) atomicOr(err_flag, 1);
    __syncthreads();
    const int nv = s_sum;
    if (blockIdx.x == 0 && tid == 0) n_valid[0] = nv;
    const float wv = (float)(1.0 / ((double)nv + 1e-12));
    const long long n = (long long)T * B;
    for (long long j = (long long)blockIdx.x * 256 + tid; j < n; j += (long long)gridDim.x * 256) {
        const int t = (int)(j / B), b = (int)(j % B);
        const int e = min(hi, clamp_len(len[b], T));
        w[j] = (t >= lo && t < e) ? wv : 0.0f;
    }
}

// out[(row0 + b) * T + t] = -ce[t * B + b] where the pass weighted the position (w != 0): the window's scores, under the parameters
// the pass ran at.  Every other element of `out` is left alone (the call zeroed it).
__global__ __launch_bounds__(256) void k_dyneval_collect(const float* __restrict__ ce, const float* __restrict__ w, int B, int T,
                                                         long long row0, float* __restrict__ out) {
    const long long n = (long long)T * B;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        if (w[j] == 0.0f) continue;
        const int t = (int)(j / B), b = (int)(j % B);
        out[(row0 + b) * T + t] = -ce[j];
    }
}

// One element of the update; every rounding is spelled out (no contraction), so the host restatement in tests/dyneval_ref.py can
// bound it operation by operation:
//   SGD: p <- (p - step * g) + decay * (pg - p)
//   RMS: r = sqrt(ms / cnt);  p <- (p - (step * g) / (r + eps)) + (decay * (pg - p)) * min(inv_decay, r / mean_rms)
// decay == 0: the pull-back term is absent (not a zero that is added).
template <bool RMS, bool DECAY>
__device__ __forceinline__ float dyn_element(float p, float pg, float g, float ms, float step, float decay, float inv_decay, float eps,
                                             float cnt, float mean_rms) {
#pragma clang fp contract(off)
    float r = 0.0f, t1 = step * g;
    if (RMS) { r = sqrtf(ms / cnt); t1 = t1 / (r + eps); }
    float q = p - t1;
    if (DECAY) {
        float t2 = decay * (pg - p);
        if (RMS) t2 = t2 * fminf(inv_decay, r / mean_rms);
        q = q + t2;
    }
    return q;
}

template <bool RMS, bool DECAY>
__device__ __forceinline__ void dyn_update_loop(const DynUpdateArgs& a, float step, float mean_rms) {
    const long long n4 = a.n >> 2;
    const float inv_decay = DECAY ? 1.0f / a.decay : 0.0f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 p = reinterpret_cast<float4*>(a.p)[i];
        const float4 g = reinterpret_cast<const float4*>(a.g)[i];
        float4 pg = p, ms = p;
        if (DECAY) pg = reinterpret_cast<const float4*>(a.pg)[i];
        if (RMS) ms = reinterpret_cast<const float4*>(a.ms)[i];
        p.x = dyn_element<RMS, DECAY>(p.x, pg.x, g.x, ms.x, step, a.decay, inv_decay, a.eps, a.count, mean_rms);
        p.y = dyn_element<RMS, DECAY>(p.y, pg.y, g.y, ms.y, step, a.decay, inv_decay, a.eps, a.count, mean_rms);
        p.z = dyn_element<RMS, DECAY>(p.z, pg.z, g.z, ms.z, step, a.decay, inv_decay, a.eps, a.count, mean_rms);
        p.w = dyn_element<RMS, DECAY>(p.w, pg.w, g.w, ms.w, step, a.decay, inv_decay, a.eps, a.count, mean_rms);
        reinterpret_cast<float4*>(a.p)[i] = p;
    }
}

// The update of one window.  The clip scale comes from the squared-norm partials exactly as k_sgd_update derives it -- every block
// from the same partials in the same order, the embedding slices' share from tail[0] under the TF1 convention -- and the kernel
// returns at once on the same conditions (the error word, tail[2..5]): a skipped pass updates nothing.
__global__ __launch_bounds__(256) void k_dyneval_update(const DynUpdateArgs a) {
    __shared__ double sh[4];
    __shared__ float s_step;
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
        const float c = a.clip > 0.0f ? (float)(clip / fmax(gnorm, clip)) : 1.0f;
        s_step = c * a.lr;
        if (a.gnorm_out != nullptr && blockIdx.x == 0) *a.gnorm_out = (float)gnorm;
    }
    __syncthreads();
    const float step = s_step;
    const bool decay = a.decay != 0.0f;
    if (a.rms) {
        const float mean_rms = *a.mean_rms;
        if (decay) dyn_update_loop<true, true>(a, step, mean_rms); else dyn_update_loop<true, false>(a, step, mean_rms);
    } else {
        if (decay) dyn_update_loop<false, true>(a, step, 0.0f); else dyn_update_loop<false, false>(a, step, 0.0f);
    }
}

// ms[i] <- ms[i] + g[i] * g[i]: two roundings per element (no contraction), the running fp32 sum of the squared gradients
__global__ __launch_bounds__(256) void k_dyneval_accumulate(float* __restrict__ ms, const float* __restrict__ g, long long n4) {
#pragma clang fp contract(off)
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        float4 m = reinterpret_cast<float4*>(ms)[i];
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        const float x = v.x * v.x, y = v.y * v.y, z = v.z * v.z, w = v.w * v.w;
        m.x = m.x + x; m.y = m.y + y; m.z = m.z + z; m.w = m.w + w;
        reinterpret_cast<float4*>(ms)[i] = m;
    }
}

// partials[c] = sum over chunk c of sqrt((double)ms[i] / count), fp64, in k_sqnorm_partials' order (n a multiple of 4)
__global__ __launch_bounds__(256) void k_dyneval_rms_partials(const float* __restrict__ ms, long long n, double count, double* __restrict__ partials) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * DYN_CHUNK;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long idx = base + 4 * (tid + 256 * i);
        if (idx + 3 < n) {
            const float4 v = *reinterpret_cast<const float4*>(ms + idx);
            s += (sqrt((double)v.x / count) + sqrt((double)v.y / count)) + (sqrt((double)v.z / count) + sqrt((double)v.w / count));
        }
    }
    s = wave_sum_d(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// *out = (float)(sum of the partials / n_logical): one block, a fixed order.  The pad elements of the flat buffer hold ms == 0 and add
// nothing to the sum; they are not counted in n_logical either.
__global__ __launch_bounds__(256) void k_dyneval_rms_finish(const double* __restrict__ partials, int n_partials, double n_logical, float* __restrict__ out) {
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double s = 0.0;
    for (int i = tid; i < n_partials; i += 256) s += partials[i];
    s = wave_sum_d(s);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (tid == 0) *out = (float)(((sh[0] + sh[1]) + (sh[2] + sh[3])) / n_logical);
}

}  // namespace

hipError_t launch_set_window(hipStream_t s, int* win, int lo, int hi) {
    if (win == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_set_window, dim3(1), dim3(64), 0, s, win, lo, hi);
    return hipGetLastError();
}

hipError_t launch_window_weights(hipStream_t s, const int* len, int B, int T, const int* win, float* w, int* n_valid, int* elen, int* err_flag) {
    if (B <= 0) return hipSuccess;
    if (len == nullptr || win == nullptr || w == nullptr || n_valid == nullptr || elen == nullptr || err_flag == nullptr) return hipErrorInvalidValue;
    const long long n = (long long)T * B;
    const int blocks = (int)std::max<long long>(1, std::min<long long>((n + 255) / 256, 64));
    hipLaunchKernelGGL(k_window_weights, dim3(blocks), dim3(256), 0, s, len, B, T, win, w, n_valid, elen, err_flag);
    return hipGetLastError();
}

hipError_t launch_dyneval_collect(hipStream_t s, const float* ce, const float* w, int B, int T, long long row0, float* out) {
    const long long n = (long long)T * B;
    if (n <= 0) return hipSuccess;
    if (ce == nullptr || w == nullptr || out == nullptr || row0 < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dyneval_collect, dim3((int)std::min<long long>((n + 255) / 256, 1024)), dim3(256), 0, s, ce, w, B, T, row0, out);
    return hipGetLastError();
}

hipError_t launch_dyneval_update(hipStream_t s, const DynUpdateArgs& a) {
    if (a.p == nullptr || a.g == nullptr || a.tail == nullptr || a.partials == nullptr || (a.n & 3) != 0) return hipErrorInvalidValue;
    if (a.decay != 0.0f && a.pg == nullptr) return hipErrorInvalidValue;
    if (a.rms && (a.ms == nullptr || a.mean_rms == nullptr || !(a.count > 0.0f) || !(a.eps > 0.0f))) return hipErrorInvalidValue;
    const long long n4 = a.n >> 2;
    int blocks = (int)((n4 + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_dyneval_update, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dyneval_accumulate(hipStream_t s, float* ms, const float* g, long long n) {
    const long long n4 = n >> 2;
    if (n4 <= 0) return hipSuccess;
    if (ms == nullptr || g == nullptr || (n & 3) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dyneval_accumulate, dim3((int)std::min<long long>((n4 + 255) / 256, 2048)), dim3(256), 0, s, ms, g, n4);
    return hipGetLastError();
}

int dyneval_rms_blocks(long long n) { return (int)((n + DYN_CHUNK - 1) / DYN_CHUNK); }

hipError_t launch_dyneval_mean_rms(hipStream_t s, const float* ms, long long n, long long count, long long n_logical, double* partials, float* out) {
    if (ms == nullptr || partials == nullptr || out == nullptr || (n & 3) != 0 || n <= 0 || count <= 0 || n_logical <= 0) return hipErrorInvalidValue;
    const int nb = dyneval_rms_blocks(n);
    hipLaunchKernelGGL(k_dyneval_rms_partials, dim3(nb), dim3(256), 0, s, ms, n, (double)count, partials);
    hipLaunchKernelGGL(k_dyneval_rms_finish, dim3(1), dim3(256), 0, s, partials, nb, (double)n_logical, out);
    return hipGetLastError();
}

}  // namespace fsmg
