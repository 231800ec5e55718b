// Carried LSTM state for the batched passes (fsmg_*_state): what stands between a decode state (fsmg_dstate_s:
// h, c [L][R][Hp], a pending token and a context ring per row) and one forward pass of the train path's kernels.
//   k_state_import      per layer, in place of the zero fills of slot 0: h, c -> Hs[l] / Cs[l] slot 0 row-major, and h once more in the
//                       hand-off layout the layer's recurrence family reads at time index 0
//   k_state_token_prep  k_token_prep_len with the state's pending token as the input of position 0 (lengths in [0, T])
//   k_state_weights     k_row_weights for one group with lengths in [0, T]
//   k_state_export      slot len[b] of Hs[l] / Cs[l] -> the state; k_state_export_ctx: the call's T context tokens into the ring
// Every hand-off layout below restates its kernel's own producer store (the `hx_out` / `hF_next` expression named beside it): the
// consumers read index 0 with the address arithmetic they read every other index with.
#include "fsmg_kernels.h"
#include <algorithm>

namespace fsmg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the three bf16 planes of the exact split the bf16-pipe recurrences hand around (lstm_xcd.hip split3: round to nearest even, the
// residual of the residual) -- the same instruction, so an imported h has the planes its producer would have stored
__device__ __forceinline__ unsigned bf16_rne(float x) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %1" : "=v"(r) : "v"(x));
    return r & 0xffffu;
}
__device__ __forceinline__ void split3(float x, unsigned (&p)[3]) {
    p[0] = bf16_rne(x);
    const float r1 = x - __uint_as_float(p[0] << 16);
    p[1] = bf16_rne(r1);
    const float r2 = r1 - __uint_as_float(p[1] << 16);
    p[2] = bf16_rne(r2);
}

__global__ __launch_bounds__(256) void k_state_import(const StateImportArgs a) {
    const int B = a.B, Hp = a.Hp, q4 = Hp >> 2;
    const long long n_rows = (long long)B * q4;
    long long n_hand = 0;
    if (a.kind == STATE_HAND_HF) n_hand = (long long)((B + 15) / 16 * 16) * q4;
    else if (a.kind == STATE_HAND_HX32) n_hand = (long long)a.ng * a.rows * q4;
    else if (a.kind == STATE_HAND_HX16) n_hand = (long long)a.ng * a.rows * (Hp >> 3);
    const int kw = Hp >> 2;                 // K range of a wave: a quarter of the hidden units
    const int rpg = (B + a.ng - 1) / (a.ng > 0 ? a.ng : 1);     // rows per weight copy (XCD, XCD pair, slice)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows + n_hand; i += (long long)gridDim.x * blockDim.x) {
        if (i < n_rows) {                   // slot 0, row-major: what the cell update, BPTT and the dKh GEMM read
            reinterpret_cast<f32x4*>(a.Hs0)[i] = reinterpret_cast<const f32x4*>(a.h)[i];
            reinterpret_cast<f32x4*>(a.Cs0)[i] = reinterpret_cast<const f32x4*>(a.c)[i];
            continue;
        }
        const long long j = i - n_rows;
        if (a.kind == STATE_HAND_HF) {
            // lstm_step.hip: hF_next[((tile * ngroups + eu / 16) * 64 + 4 * (eu & 12) + row % 16) * 4 + eu % 4], pad rows zeros
            const int bp = (int)(j / q4), u0 = 4 * (int)(j % q4);
            const f32x4 v = bp < B ? *reinterpret_cast<const f32x4*>(a.h + (size_t)bp * Hp + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
            reinterpret_cast<f32x4*>(a.hand)[((size_t)(bp >> 4) * (Hp >> 4) + (u0 >> 4)) * 64 + 4 * (u0 & 12) + (bp & 15)] = v;
        } else if (a.kind == STATE_HAND_HX32) {
            // k_lstm_fwd_xcd / _slice / _pair(_chains): the cell thread of (row 4 rg + ci of its copy, units 16 cu + 4 cbb ...) stores
            // hx_out = (((copy * 4 + w) * RG + rg) * NQ + q) * 64 + 16 * (cu & 3) + 4 * cbb + ci, w / q = the consumer wave / fragment of
            // unit 16 cu (a wave's K range is Hp / 4 units in NQ fragments of 64)
            const int u0 = 4 * (int)(j % q4);
            const int lrow = (int)((j / q4) % a.rows), g = (int)(j / ((long long)q4 * a.rows));
            const int row = g * rpg + lrow;
            const bool act = lrow < rpg && row < B;
            const f32x4 v = act ? *reinterpret_cast<const f32x4*>(a.h + (size_t)row * Hp + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
            const int w = u0 / kw, q = (u0 % kw) >> 6, rg = lrow >> 2, ci = lrow & 3;
            reinterpret_cast<f32x4*>(a.hand)[((((size_t)g * 4 + w) * (a.rows >> 2) + rg) * a.nq + q) * 64 + 16 * ((u0 >> 4) & 3) + (u0 & 12) + ci] = v;
        } else {
            // k_lstm_fwd_xcd16 / _pair16: eight units of one row and plane are one word,
            // hx_out = ((copy * 4 + w) * 3 KS + plane * KS + k step) * (HXR * 4) + row * 4 + k group, unit u -> w = u / (Hp / 4),
            // k step = u % (Hp / 4) / 32, k group = u % 32 / 8; component j = {unit 2 j low half, unit 2 j + 1 high half}
            const int o8 = Hp >> 3;
            const int u0 = 8 * (int)(j % o8);
            const int lrow = (int)((j / o8) % a.rows), g = (int)(j / ((long long)o8 * a.rows));
            const int row = g * rpg + lrow;
            const bool act = lrow < rpg && row < B;
            unsigned pl[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            if (act) {
                const float* src = a.h + (size_t)row * Hp + u0;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    unsigned p[3];
                    split3(src[e], p);
#pragma unroll
                    for (int k = 0; k < 3; ++k) pl[k][e >> 1] |= p[k] << (16 * (e & 1));
                }
            }
            const int w = u0 / kw, ks = (u0 % kw) >> 5, kg = (u0 & 31) >> 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const size_t word = (((size_t)g * 4 + w) * (3 * a.nq) + k * a.nq + ks) * ((size_t)a.rows * 4) + lrow * 4 + kg;
                reinterpret_cast<uint4*>(a.hand)[word] = make_uint4(pl[k][0], pl[k][1], pl[k][2], pl[k][3]);
            }
        }
    }
}

__device__ __forceinline__ int state_len(const int* __restrict__ len, int b, int T) { return len ? min(max(len[b], 0), T) : T; }

// tokens [B][T] -> X, Y (time-major) as k_token_prep_len leaves them, except that a row with len[b] > 0 reads its state's pending token
// (ctx[b][kept]) at position 0 -- and the occurrence table counts THAT id at position b, or the embedding gradient of the row would go
// to the start word's row.  Integer atomics: the table does not depend on their order.
__global__ __launch_bounds__(256) void k_state_token_prep(const int* __restrict__ tokens, int B, int T, int vocab, int start_word,
                                                          const int* __restrict__ len, const int* __restrict__ ctx, int ldctx, int kept,
                                                          int* __restrict__ X, int* __restrict__ Y, int* __restrict__ err_flag,
                                                          int* __restrict__ tok_first, int* __restrict__ tok_count) {
    const long long total = (long long)B * T;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / T), t = (int)(i % T);
        int tok = tokens[i];
        if (tok < 0 || tok >= vocab) {
            atomicOr(err_flag, 1);
            tok = min(max(tok, 0), vocab - 1);
        }
        const int l = state_len(len, b, T);
        Y[(long long)t * B + b] = t < l ? tok : 0;
        if (t + 1 < T) {
            const int xin = t + 1 < l ? tok : start_word;
            const long long pos = (long long)(t + 1) * B + b;
            X[pos] = xin;
            if (tok_first != nullptr) { atomicMin(tok_first + xin, (int)pos); atomicAdd(tok_count + xin, 1); }
        }
        if (t == 0) {
            int x0 = l > 0 ? ctx[(long long)b * ldctx + kept] : start_word;
            if (x0 < 0 || x0 > vocab) { atomicOr(err_flag, 1); x0 = start_word; }
            X[b] = x0;
            if (tok_first != nullptr) { atomicMin(tok_first + x0, b); atomicAdd(tok_count + x0, 1); }
        }
    }
}

// k_row_weights for one group of B rows with lengths in [0, T]: a row of length 0 has no scored position
__global__ __launch_bounds__(256) void k_state_weights(const int* __restrict__ len, int B, int T, float* __restrict__ w, int* __restrict__ n_valid) {
    __shared__ int s_sum;
    const int tid = threadIdx.x;
    if (tid == 0) s_sum = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < B; i += 256) mine += state_len(len, i, T);
    if (mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    const int nv = s_sum;
    if (blockIdx.x == 0 && tid == 0) n_valid[0] = nv;
    const float wv = (float)(1.0 / ((double)nv + 1e-12));
    const long long n = (long long)T * B;
    for (long long j = (long long)blockIdx.x * 256 + tid; j < n; j += (long long)gridDim.x * 256) {
        const int t = (int)(j / B), b = (int)(j % B);
        w[j] = t < state_len(len, b, T) ? wv : 0.0f;
    }
}

// the state after the pass: row b of layer l takes slot len[b] of Hs[l] / Cs[l], bit for bit (len[b] == 0: the row keeps what it has).
// Nothing is written when the pass raised a flag (time-out, token range, softmax range): the step is skipped or repeated, and the
// repeat imports the state this pass imported.
__global__ __launch_bounds__(256) void k_state_export(const float* __restrict__ Hs, const float* __restrict__ Cs, int B, int Hp, int T,
                                                      const int* __restrict__ len, float* __restrict__ h, float* __restrict__ c,
                                                      const int* __restrict__ err_flag) {
    if (*err_flag != 0) return;
    const int q4 = Hp >> 2;
    const long long n = (long long)B * q4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / q4);
        const int l = state_len(len, b, T);
        if (l == 0) continue;
        const size_t src = ((size_t)l * B) * q4 + i;
        reinterpret_cast<f32x4*>(h)[i] = reinterpret_cast<const f32x4*>(Hs)[src];
        reinterpret_cast<f32x4*>(c)[i] = reinterpret_cast<const f32x4*>(Cs)[src];
    }
}

// The ring after the pass, one block per row: the context gains y[t] = x[t] for t < len, the last real token (x[len - 1], or the old
// pending token when len == 0) repeated behind it; ctx[b][1 .. keep] = the last `keep` tokens of (old context, y), the last one pending.
// In place: a slot's source never lies below it, chunks ascend, and a chunk is read whole before it is written.
__global__ __launch_bounds__(256) void k_state_export_ctx(const int* __restrict__ tokens, int T, int vocab, const int* __restrict__ len,
                                                          int* __restrict__ ctx, int ldctx, int kept, int keep,
                                                          const int* __restrict__ err_flag) {
    if (*err_flag != 0) return;
    const int b = blockIdx.x, tid = threadIdx.x;
    int* row = ctx + (long long)b * ldctx;
    const int* x = tokens + (long long)b * T;
    const int l = state_len(len, b, T);
    int last = l > 0 ? x[l - 1] : row[kept];
    if (l > 0) last = min(max(last, 0), vocab - 1);
    const int shift = kept + T - keep;          // slot 1 + j takes element shift + j of (old context [kept], y [T])
    for (int base = 0; base < keep; base += 256) {
        const int j = base + tid;
        int v = 0;
        if (j < keep) {
            const int s = shift + j;
            if (s < kept) v = row[1 + s];
            else { const int t = s - kept; v = t < l ? min(max(x[t], 0), vocab - 1) : last; }
        }
        __syncthreads();
        if (j < keep) row[1 + j] = v;
        __syncthreads();
    }
}

inline int grid_for(long long n, int cap = 1024) { return (int)std::min<long long>(std::max<long long>((n + 255) / 256, 1), cap); }

}  // namespace

hipError_t launch_state_import(hipStream_t s, const StateImportArgs& a) {
    if (a.B <= 0 || a.Hp <= 0 || (a.Hp & 15) != 0) return hipErrorInvalidValue;
    if (a.kind != STATE_HAND_NONE && a.hand == nullptr) return hipErrorInvalidValue;
    if ((a.kind == STATE_HAND_HX32 || a.kind == STATE_HAND_HX16) && (a.ng <= 0 || a.nq <= 0 || a.rows <= 0 || (a.rows & 3) != 0 || (a.Hp & 255) != 0))
        return hipErrorInvalidValue;
    const long long n = (long long)std::max(a.B, a.ng * a.rows) * (a.Hp >> 2) * 2;
    hipLaunchKernelGGL(k_state_import, dim3(grid_for(n)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_state_token_prep(hipStream_t s, const int* tokens, int B, int T, int vocab, int start_word, const int* len, const int* ctx,
                                   int ldctx, int kept, int* X, int* Y, int* err_flag, int* tok_first, int* tok_count) {
    if (B <= 0 || T <= 0 || kept < 0 || kept >= ldctx) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_state_token_prep, dim3(grid_for((long long)B * T)), dim3(256), 0, s, tokens, B, T, vocab, start_word, len, ctx, ldctx,
                       kept, X, Y, err_flag, tok_first, tok_count);
    return hipGetLastError();
}

hipError_t launch_state_weights(hipStream_t s, const int* len, int B, int T, float* w, int* n_valid) {
    if (B <= 0 || T <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_state_weights, dim3(grid_for((long long)B * T, 64)), dim3(256), 0, s, len, B, T, w, n_valid);
    return hipGetLastError();
}

hipError_t launch_state_export(hipStream_t s, const float* Hs, const float* Cs, int B, int Hp, int T, const int* len, float* h, float* c,
                               const int* err_flag) {
    if (B <= 0 || Hp <= 0 || (Hp & 3) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_state_export, dim3(grid_for((long long)B * (Hp >> 2))), dim3(256), 0, s, Hs, Cs, B, Hp, T, len, h, c, err_flag);
    return hipGetLastError();
}

hipError_t launch_state_export_ctx(hipStream_t s, const int* tokens, int B, int T, int vocab, const int* len, int* ctx, int ldctx, int kept,
                                   int keep, const int* err_flag) {
    if (B <= 0 || T <= 0 || kept < 0 || keep < 0 || kept >= ldctx || keep >= ldctx || keep > kept + T) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_state_export_ctx, dim3(B), dim3(256), 0, s, tokens, T, vocab, len, ctx, ldctx, kept, keep, err_flag);
    return hipGetLastError();
}

}  // namespace fsmg
