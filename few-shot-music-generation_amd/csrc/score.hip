// Scoring kernel of fsmg_score (include/fsmg.h): per logits row the target's log-probability and rank, the predictive
// entropy and the argmax.  HBM bound: one 256-thread block (four wave64) per row, 16-byte loads, the row read once where it fits
// the registers.  No atomics; reductions in a fixed order (wave shuffles, then four LDS words), so a row's bits do not depend on
// where or when its block runs.
#include "fsmg_kernels.h"

namespace fsmg {
namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// the float4 at columns [v, v + 4) of a row, pad columns (>= n_vocab, and a whole float4 past ld) as -inf
__device__ __forceinline__ float4 load_cols(const float* __restrict__ row, int v, int ld, int n_vocab) {
    float4 x = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (v < ld) {                                       // ld is a multiple of 4 and >= n_vocab: the whole float4 is in bounds
        const float4 q = *reinterpret_cast<const float4*>(row + v);
        x.x = (v + 0 < n_vocab) ? q.x : -INFINITY; x.y = (v + 1 < n_vocab) ? q.y : -INFINITY;
        x.z = (v + 2 < n_vocab) ? q.z : -INFINITY; x.w = (v + 3 < n_vocab) ? q.w : -INFINITY;
    }
    return x;
}
__device__ __forceinline__ float max4(float m, const float4& x) { return fmaxf(fmaxf(m, fmaxf(x.x, x.y)), fmaxf(x.z, x.w)); }

// what a thread gathers over its columns once the row maximum m and the target logit xt are known
struct Acc {
    float s = 0.0f, w = 0.0f;       // sum exp(z - m), sum exp(z - m) * (z - m)
    int rank = 0;                   // #{z_v > z_y} + #{v < y : z_v == z_y}
};
// e * d with a -inf column (e == 0, d == -inf) contributing -0, not NaN; a NaN column still gives NaN through e
__device__ __forceinline__ float ent_term(float e, float d) { return e * fmaxf(d, -3.402823466e+38f); }
__device__ __forceinline__ void gather4(Acc& a, const float4& x, int v, float m, float xt, int t) {
    const float d0 = x.x - m, d1 = x.y - m, d2 = x.z - m, d3 = x.w - m;
    const float e0 = expf(d0), e1 = expf(d1), e2 = expf(d2), e3 = expf(d3);
    a.s += (e0 + e1) + (e2 + e3);
    a.w += (ent_term(e0, d0) + ent_term(e1, d1)) + (ent_term(e2, d2) + ent_term(e3, d3));
    // columns in front of the target count from a tie on, columns behind it only when larger (the pad columns, -inf, lie behind it)
    if (v + 3 < t) a.rank += (int)(x.x >= xt) + (int)(x.y >= xt) + (int)(x.z >= xt) + (int)(x.w >= xt);
    else if (v > t) a.rank += (int)(x.x > xt) + (int)(x.y > xt) + (int)(x.z > xt) + (int)(x.w > xt);
    else a.rank += (int)(x.x > xt || (x.x == xt && v + 0 < t)) + (int)(x.y > xt || (x.y == xt && v + 1 < t)) +
                   (int)(x.z > xt || (x.z == xt && v + 2 < t)) + (int)(x.w > xt || (x.w == xt && v + 3 < t));
}
// the lowest of the four columns holding m, or INT_MAX
__device__ __forceinline__ int first_hit(const float4& x, int v, float m) {
    return x.x == m ? v : x.y == m ? v + 1 : x.z == m ? v + 2 : x.w == m ? v + 3 : 0x7FFFFFFF;
}

// NV > 0: the row lives in NV float4 per thread (ld <= NV * 1024), read once.  NV == 0: streaming, the row is read twice (the second
// read of a 200 KB row is an L2 hit) with the same per-element arithmetic in the same order.
// Row r = t * B + b of the time-major logits; the outputs are written transposed, [b][t].  A null output is not stored.
template <int NV>
__global__ __launch_bounds__(256) void k_score_rows(const float* __restrict__ logits, int ld, int n_vocab, const int* __restrict__ tgt,
                                                    int B, int T, float* __restrict__ out_lp, int* __restrict__ out_rank,
                                                    float* __restrict__ out_ent, int* __restrict__ out_arg) {
    __shared__ float sh_m[4], sh_s[4], sh_w[4];
    __shared__ int sh_rank[4], sh_arg[4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (long long)r * ld;
    const int t = tgt[r];                               // in [0, n_vocab): the token staging clamps what it flags
    constexpr int NX = NV > 0 ? NV : 1;
    float4 x[NX];
    float tm = -INFINITY;                               // this thread's maximum: only a thread that holds m looks for its column
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            x[i] = load_cols(row, 4 * tid + 1024 * i, ld, n_vocab);
            tm = max4(tm, x[i]);
        }
    } else {
        for (int v = 4 * tid; v < ld; v += 1024) tm = max4(tm, load_cols(row, v, ld, n_vocab));
    }
    float m = wave_max(tm);
    if (lane == 0) sh_m[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
    const float xt = row[t];
    Acc a;
    int arg = 0x7FFFFFFF;
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NX; ++i) gather4(a, x[i], 4 * tid + 1024 * i, m, xt, t);
        if (tm == m) {
#pragma unroll
            for (int i = NX - 1; i >= 0; --i) arg = min(arg, first_hit(x[i], 4 * tid + 1024 * i, m));
        }
    } else {
        for (int v = 4 * tid; v < ld; v += 1024) gather4(a, load_cols(row, v, ld, n_vocab), v, m, xt, t);
        if (tm == m)
            for (int v = 4 * tid; v < ld && arg == 0x7FFFFFFF; v += 1024) arg = first_hit(load_cols(row, v, ld, n_vocab), v, m);
    }
    a.s = wave_sum(a.s); a.w = wave_sum(a.w);
    a.rank = wave_sum_i(a.rank); arg = wave_min_i(arg);
    if (lane == 0) { sh_s[wave] = a.s; sh_w[wave] = a.w; sh_rank[wave] = a.rank; sh_arg[wave] = arg; }
    __syncthreads();
    if (tid != 0) return;
    const float S = (sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]);
    const float W = (sh_w[0] + sh_w[1]) + (sh_w[2] + sh_w[3]);
    const float logS = logf(S);
    const long long o = (long long)(r % B) * T + r / B;
    if (out_lp != nullptr) out_lp[o] = xt - (m + logS);
    if (out_ent != nullptr) out_ent[o] = logS - W / S;
    if (out_rank != nullptr) out_rank[o] = min((sh_rank[0] + sh_rank[1]) + (sh_rank[2] + sh_rank[3]), n_vocab - 1);
    if (out_arg != nullptr) {
        const int best = min(min(sh_arg[0], sh_arg[1]), min(sh_arg[2], sh_arg[3]));
        out_arg[o] = best < n_vocab ? best : 0;           // (a row without a comparable maximum: NaN everywhere)
    }
}

}  // namespace

hipError_t launch_score_rows(hipStream_t s, const float* logits, int ld, int rows, int n_vocab, const int* tgt, int B, int T,
                             float* out_lp, int* out_rank, float* out_ent, int* out_arg) {
    if (rows <= 0) return hipSuccess;
    if (ld < n_vocab || (ld & 3) != 0 || B <= 0 || rows != B * T) return hipErrorInvalidValue;
#define FSMG_SCORE_LAUNCH(NV) \
    hipLaunchKernelGGL((k_score_rows<NV>), dim3(rows), dim3(256), 0, s, logits, ld, n_vocab, tgt, B, T, out_lp, out_rank, out_ent, out_arg)
    if (ld <= 1024) FSMG_SCORE_LAUNCH(1);
    else if (ld <= 3 * 1024) FSMG_SCORE_LAUNCH(3);
    else if (ld <= 6 * 1024) FSMG_SCORE_LAUNCH(6);
    else if (ld <= SCORE_REG_COLS) FSMG_SCORE_LAUNCH(10);
    else FSMG_SCORE_LAUNCH(0);
#undef FSMG_SCORE_LAUNCH
    return hipGetLastError();
}

}  // namespace fsmg
