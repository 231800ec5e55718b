// Batched sampling decode (fsmg_generate, DESIGN.md "Batched generation"): one LSTM position for B independent rows per
// (L cell launches + logits + pick).  Generation is weight-streaming -- one position reads [Kx;Kh] of every layer and softmax_w
// whatever B is -- so the GEMV kernels load their 16-column weight tile straight to VGPRs and loop the row tiles of the
// workgroup over it; the products run on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation).
//
// Row independence: every output element is an fp32 fma chain over k in an order fixed by the kernel's shape (in_dim, Hp),
// and the cross-wave sums / the pick's reductions have a fixed tree: nothing depends on B or on the other rows.
#include <math.h>

#include <algorithm>
#include <atomic>

#include "fsmg_kernels.h"

namespace fsmg {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GEN_THREADS = 256;   // 4 waves
constexpr int GEN_ROWS = 64;       // rows per workgroup: 4 row tiles of 16 (grid.y covers the rest)
constexpr int GEN_CH = 16;         // k per lane held in registers at a time
constexpr int PICK_THREADS = 1024;
constexpr int PICK_LDS_FLOATS = 32 * 1024;   // rows up to 128 KiB are staged in LDS
constexpr int BEAM_MAX_W = 64;
constexpr int SEL_THREADS = 1024;

// Partial products of one 16-column weight tile with up to 4 row tiles over one K segment of n rows (n % 16 == 0).
// The segment is split into 16 slots of m = n / 16 consecutive k (slot = 4 * wave + lane group); lane (c = l & 15, g = l >> 4)
// holds W[k][c] as the MFMA's B operand and act[row c of the tile][k] as its A operand, so one MFMA sums 4 k of 4 slots.
// `w` points at column c of the tile (nullptr: a column past the end, read as zeros); ap[rt] at the segment's row of the lane's
// row in tile rt (nullptr: a row past B).  acc[rt] is the 16 x 16 D tile (col = l & 15, row = 4 * (l >> 4) + reg).
__device__ __forceinline__ void gemv_segment(const float* __restrict__ w, long long ldw, int n, const float* const (&ap)[4], int nrt,
                                             f32x4 (&acc)[4]) {
    const int m = n >> 4;
    const int slot = (threadIdx.x >> 6) * 4 + ((threadIdx.x & 63) >> 4);
    const int kb = slot * m;
    for (int c0 = 0; c0 < m; c0 += GEN_CH) {
        float wr[GEN_CH];
#pragma unroll
        for (int s = 0; s < GEN_CH; ++s) wr[s] = (w != nullptr && c0 + s < m) ? w[(long long)(kb + c0 + s) * ldw] : 0.0f;
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) {
            if (rt >= nrt) break;
            const float* a = ap[rt];
            float av[GEN_CH];
#pragma unroll
            for (int s = 0; s < GEN_CH; ++s) av[s] = (a != nullptr && c0 + s < m) ? a[kb + c0 + s] : 0.0f;
#pragma unroll
            for (int s = 0; s < GEN_CH; ++s)
                if (c0 + s < m) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], wr[s], acc[rt], 0, 0, 0);
        }
    }
}

// the four waves' partial tiles -> LDS [wave][row][col] (col padded to 17: the transposed reads of the epilogue)
__device__ __forceinline__ void store_partials(float (&part)[4][GEN_ROWS][17], const f32x4 (&acc)[4], int nrt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        if (rt >= nrt) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][rt * 16 + 4 * (lane >> 4) + r][lane & 15] = acc[rt][r];
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// One LSTM layer at one position for rows [64 * blockIdx.y, +64) and unit block nb = blockIdx.x (units 4nb..4nb+3, packed
// columns 16nb..16nb+15 of the gate-interleaved [Kx;Kh]).  Layer 0 (emb != nullptr) gathers its x rows from the embedding by
// the device-resident token tok[r * ldtok + pos]; other layers read x = the layer below's h at this position ([B][Hp]).
__global__ __launch_bounds__(GEN_THREADS) void k_gen_cell(const float* __restrict__ Kx, int in_dim, const float* __restrict__ Kh,
                                                          const float* __restrict__ bias, int Hp, const float* __restrict__ emb, int ldemb,
                                                          const int* __restrict__ tok, int ldtok, int pos, const float* __restrict__ x,
                                                          const float* __restrict__ h_in, float* __restrict__ h_out, float* __restrict__ c,
                                                          int B) {
    __shared__ float part[4][GEN_ROWS][17];
    const int nb = blockIdx.x, r0 = blockIdx.y * GEN_ROWS;
    const int lane = threadIdx.x & 63;
    const int G4 = 4 * Hp;
    const int nrt = min(4, (B - r0 + 15) >> 4);
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* ap[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int r = r0 + rt * 16 + (lane & 15);
        ap[rt] = r >= B ? nullptr : emb != nullptr ? emb + (long long)tok[(long long)r * ldtok + pos] * ldemb : x + (long long)r * Hp;
    }
    gemv_segment(Kx + 16 * nb + (lane & 15), G4, in_dim, ap, nrt, acc);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int r = r0 + rt * 16 + (lane & 15);
        ap[rt] = r < B ? h_in + (long long)r * Hp : nullptr;
    }
    gemv_segment(Kh + 16 * nb + (lane & 15), G4, Hp, ap, nrt, acc);
    store_partials(part, acc, nrt);
    __syncthreads();
    const int row = threadIdx.x >> 2, uu = threadIdx.x & 3, r = r0 + row;
    if (r >= B) return;
    float z[4];
#pragma unroll
    for (int gi = 0; gi < 4; ++gi) {
        const int col = 4 * gi + uu;
        float t = part[0][row][col];
        t += part[1][row][col];
        t += part[2][row][col];
        t += part[3][row][col];
        z[gi] = t + bias[16 * nb + col];
    }
    // gates i, j, f, o; forget bias 1 (BasicLSTMCell(forget_bias=1.))
    const long long u = (long long)r * Hp + 4 * nb + uu;
    const float si = sigmoidf_(z[0]), tj = tanhf(z[1]), sf = sigmoidf_(z[2] + 1.0f), so = sigmoidf_(z[3]);
    const float cn = c[u] * sf + si * tj;
    c[u] = cn;
    h_out[u] = tanhf(cn) * so;
}

// logits[r][v] = h[r] . W[:, v] + bias[v] for v < ncols; column tile 16 * blockIdx.x, rows 64 * blockIdx.y
__global__ __launch_bounds__(GEN_THREADS) void k_gen_logits(const float* __restrict__ W, int ldw, const float* __restrict__ bias, int ncols,
                                                            const float* __restrict__ h, int Hp, int B, float* __restrict__ logits, int ldl) {
    __shared__ float part[4][GEN_ROWS][17];
    const int col0 = 16 * blockIdx.x, r0 = blockIdx.y * GEN_ROWS;
    const int lane = threadIdx.x & 63;
    const int nrt = min(4, (B - r0 + 15) >> 4);
    f32x4 acc[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) acc[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* ap[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int r = r0 + rt * 16 + (lane & 15);
        ap[rt] = r < B ? h + (long long)r * Hp : nullptr;
    }
    const int cl = col0 + (lane & 15);
    gemv_segment(cl < ncols ? W + cl : nullptr, ldw, Hp, ap, nrt, acc);
    store_partials(part, acc, nrt);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GEN_ROWS * 16 / GEN_THREADS; ++i) {
        const int idx = threadIdx.x + GEN_THREADS * i, row = idx >> 4, col = idx & 15;
        const int r = r0 + row, v = col0 + col;
        if (r >= B || v >= ncols) continue;
        float t = part[0][row][col];
        t += part[1][row][col];
        t += part[2][row][col];
        t += part[3][row][col];
        logits[(long long)r * ldl + v] = t + bias[v];
    }
}

// ---------------------------------------------------------------- the pick
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned lo0 = 0xD2511F53u * ctr.x, hi0 = __umulhi(0xD2511F53u, ctr.x);
        const unsigned lo1 = 0xCD9E8D57u * ctr.z, hi1 = __umulhi(0xCD9E8D57u, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += 0x9E3779B9u; key.y += 0xBB67AE85u;
    }
    return ctr;
}

// -log(-log(u)), u = ((x >> 8) + 0.5) * 2^-24 in (0, 1).  Every u and 1 - u of this grid is exact in fp32, so -log(u) is taken
// as log1p(-(1 - u)) where u >= 1/2 (no cancellation next to 1) and the result is good to a few fp32 ulps.
__device__ __forceinline__ float gumbel_of(unsigned x) {
    const unsigned i = x >> 8;
    float nl;
    if (i < (1u << 23)) nl = -logf(((float)i + 0.5f) * 0x1p-24f);
    else nl = -log1pf(-(((float)((1u << 24) - i) - 0.5f) * 0x1p-24f));
    return -logf(nl);
}

// order-preserving uint key of a float (larger float -> larger key)
__device__ __forceinline__ unsigned fkey(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// radix_select's histogram and result: T = int for counts (PickShared), 64-bit fixed point for the top-p masses
template <class T>
struct RadixShared {
    T hist[256];
    T left;
    unsigned prefix;
};

struct PickShared {
    float fv[PICK_THREADS / 64];
    int iv[PICK_THREADS / 64];
    double dv[PICK_THREADS / 64];
    RadixShared<int> rs;
};

// block-wide (max, lowest index) -- every thread gets the result
__device__ __forceinline__ void block_argmax(PickShared& sh, float& v, int& i) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sh.fv[w] = v; sh.iv[w] = i; }
    __syncthreads();
    v = sh.fv[0]; i = sh.iv[0];
    for (int k = 1; k < PICK_THREADS / 64; ++k)
        if (sh.fv[k] > v || (sh.fv[k] == v && sh.iv[k] < i)) { v = sh.fv[k]; i = sh.iv[k]; }
}
__device__ __forceinline__ double block_sum(PickShared& sh, double s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.dv[w] = s;
    __syncthreads();
    double t = 0.0;
    for (int k = 0; k < PICK_THREADS / 64; ++k) t += sh.dv[k];
    return t;
}

// The row's maximum (lowest index on ties; column 0 when no logit exceeds -inf) and logsumexp over ncols logits: one sweep that
// also stages the row in LDS (STAGED), then the double-accumulated sum of expf(logit - max) over a fixed tree.  Shared by
// k_gen_pick and k_beam_rowtop, so that fsmg_generate's and fsmg_beam_search's log-probs are the same numbers.
template <bool STAGED>
__device__ __forceinline__ float row_max_lse(PickShared& sh, const float* __restrict__ row, float* srow, int ncols, float& mx, int& mi) {
    const int tid = threadIdx.x;
    // staging and the row maximum in one sweep, 8 loads in flight per thread (the sweep is latency-bound at small B)
    // the index starts at column 0, so that a row without a comparable logit (all NaN) still yields a column
    mx = -INFINITY; mi = 0;
    for (int v0 = tid; v0 < ncols; v0 += 8 * PICK_THREADS) {
        float l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) l[j] = v0 + j * PICK_THREADS < ncols ? row[v0 + j * PICK_THREADS] : -INFINITY;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int v = v0 + j * PICK_THREADS;
            if (v >= ncols) break;
            if (STAGED) srow[v] = l[j];
            if (l[j] > mx || (l[j] == mx && v < mi)) { mx = l[j]; mi = v; }
        }
    }
    block_argmax(sh, mx, mi);          // (its barriers also order the staging stores before the reads below)
    double se = 0.0;
    for (int v = tid; v < ncols; v += PICK_THREADS) se += (double)expf((STAGED ? srow[v] : row[v]) - mx);
    se = block_sum(sh, se);
    return mx + (float)log(se);
}

// MSB-first radix select over the 8-bit digits of key_at(v), v < ncols, each column weighing weight_at(v) (0: not counted): the
// largest key x such that the columns with key >= x weigh at least target(Z), Z the weight of all of them (seen by the first pass).
// rs.left is then the weight of the columns with exactly that key that complete the target.  The weights are integers (counts, or
// the top-p masses in fixed point), so the histograms' sums do not depend on the order the threads arrive in.  Key 0 when no key
// reaches the target (Z = 0).
template <class T, class KeyAt, class WeightAt, class Target>
__device__ __forceinline__ unsigned radix_select(RadixShared<T>& rs, int ncols, KeyAt key_at, WeightAt weight_at, Target target) {
    const int tid = threadIdx.x;
    if (tid == 0) rs.prefix = 0u;
    unsigned mask = 0u;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) rs.hist[tid] = T(0);
        __syncthreads();
        const unsigned prefix = rs.prefix;
        for (int v = tid; v < ncols; v += PICK_THREADS) {
            const unsigned key = key_at(v);
            if ((key & mask) != prefix) continue;
            const T w = weight_at(v);
            if (w) atomicAdd(&rs.hist[(key >> shift) & 255u], w);
        }
        __syncthreads();
        if (tid < 64) {       // wave 0: lane l owns digits 255 - 4l .. 252 - 4l; weights from the top digit down
            T cnt[4], s = T(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { cnt[j] = rs.hist[255 - 4 * tid - j]; s += cnt[j]; }
            T incl = s;
            for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(incl, o); if (tid >= o) incl += y; }
            T before = incl - s;
            const T kl = shift == 24 ? target(__shfl(incl, 63)) : rs.left;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (before < kl && kl <= before + cnt[j]) {
                    rs.prefix = prefix | ((unsigned)(255 - 4 * tid - j) << shift);
                    rs.left = kl - before;
                }
                before += cnt[j];
            }
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    return rs.prefix;
}

// Gumbel-max over the columns with val(v) >= thr: the argmax of val(v) / temperature + Gumbel(Philox(key = seed, ctr = (v >> 2, t,
// b, 0))), lowest index on ties; `start` when no column scores above -inf
template <class ValAt>
__device__ __forceinline__ int gumbel_max(PickShared& sh, int ncols, float thr, float temperature, unsigned seed_lo, unsigned seed_hi,
                                          int t, int b, int start, ValAt val) {
    const uint2 key = make_uint2(seed_lo, seed_hi);
    float bs = -INFINITY; int bi = start;
    for (int q = threadIdx.x; 4 * q < ncols; q += PICK_THREADS) {
        const uint4 x = philox4x32_10(make_uint4((unsigned)q, (unsigned)t, (unsigned)b, 0u), key);
        const unsigned xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = 4 * q + j;
            if (v >= ncols) break;
            const float l = val(v);
            if (!(l >= thr)) continue;
            const float s = l / temperature + gumbel_of(xs[j]);
            if (s > bs || (s == bs && v < bi)) { bs = s; bi = v; }
        }
    }
    block_argmax(sh, bs, bi);
    return bi;
}

// the picked token of row b at generated position t -> the token buffer (the next position's input) and out_tok [b][t]; its raw
// log-prob row[token] - lse -> out_lp [b][t].  The token gathers an embedding row at the next position: never outside [0, ncols).
__device__ __forceinline__ void write_pick(int best, const float* __restrict__ row, float lse, int ncols, int b, int t, int* __restrict__ tok,
                                           int ldtok, int pos_out, int* __restrict__ out_tok, float* __restrict__ out_lp, int num) {
    best = min(max(best, 0), ncols - 1);
    if (threadIdx.x == 0) {
        tok[(long long)b * ldtok + pos_out] = best;
        out_tok[(long long)b * num + t] = best;
        out_lp[(long long)b * num + t] = row[best] - lse;
    }
}

// One row per workgroup.  Token = argmax over the allowed set of logit / T + Gumbel(Philox(key = seed, ctr = (v >> 2, ctr_t, b, 0))),
// lowest index on ties; T == 0 or top_k == 1: argmax of the logits.  ctr_t is the Philox position, t the output index: equal in a
// one-shot call, ctr_t = n_gen + t when the call continues a decode state.  Allowed set: logit >= the top_k-th largest logit (radix
// select on order-preserving keys), every column when top_k is 0 or ncols.  Writes the token into the token buffer (the next
// position's input), out_tok / out_lp [b][t], lp = logit_tok - logsumexp(all ncols logits).
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_gen_pick(const float* __restrict__ logits, int ldl, int ncols, float temperature, int top_k,
                                                           unsigned seed_lo, unsigned seed_hi, int t, int ctr_t, int* __restrict__ tok,
                                                           int ldtok, int pos_out, int* __restrict__ out_tok, float* __restrict__ out_lp,
                                                           int num) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    const int b = blockIdx.x;
    const float* row = logits + (long long)b * ldl;
    auto val = [&](int v) -> float { return STAGED ? srow[v] : row[v]; };

    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);

    int best = mi;
    if (temperature > 0.0f && top_k != 1) {
        float thr = -INFINITY;
        if (top_k > 1 && top_k < ncols)
            thr = key_float(radix_select(sh.rs, ncols, [&](int v) { return fkey(val(v)); }, [](int) { return 1; }, [&](int) { return top_k; }));
        best = gumbel_max(sh, ncols, thr, temperature, seed_lo, seed_hi, ctr_t, b, 0, val);
    }
    write_pick(best, row, lse, ncols, b, t, tok, ldtok, pos_out, out_tok, out_lp, num);
}

// token buffer row b: [start, primer[b / rows_per_primer][0..P-1]]; *err = 1 for a primer id outside [0, vocab)
__global__ void k_gen_primer(const int* __restrict__ primer, int B, int P, int vocab, int start, int* __restrict__ tok, int ldtok,
                             int* __restrict__ err, int rows_per_primer) {
    const long long n = (long long)B * (P + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / (P + 1)), p = (int)(i % (P + 1));
        int w = start;
        if (p > 0) {
            w = primer[(long long)(b / rows_per_primer) * P + p - 1];
            if (w < 0 || w >= vocab) { atomicOr(err, 1); w = start; }
        }
        tok[(long long)b * ldtok + p] = w;
    }
}

// ---------------------------------------------------------------- beam search (fsmg_beam_search, DESIGN.md "Beam search")
// Rows r = g * W + j (group g, slot j).  Per generated position: k_beam_rowtop (each row's W best candidates), k_beam_select (the
// group's W best of its W x W), k_beam_reorder (each slot takes its parent's h and c).  A candidate (j, v) has lp = logit_v - lse_j
// and score s = cum_j + lp; the ranking is s descending, then j ascending, then logit descending, then v ascending, NaN below -inf.
// Within a row lp and s are nondecreasing in the logit, so a row's order is (logit descending, v ascending): a row's own W best
// are the only ones of its candidates that can enter the group's W best.

// order-preserving key of a score or logit for the beam ranking: NaN lowest (below -inf), -0 ranked equal to +0
__device__ __forceinline__ unsigned beam_key(float f) { return f != f ? 0u : fkey(f == 0.0f ? 0.0f : f); }

// One row per workgroup: lse (the sweep k_gen_pick runs), then the row's min(W, ncols) best columns in rank order ->
// cand_*[r * W + rank] (cand_v = -1 pads a row with fewer than W columns).  The W-th key comes from the radix select; the columns
// above it are gathered in any order and the boundary ties by an ordered scan (lowest columns first), then ranked in LDS.
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_beam_rowtop(const float* __restrict__ logits, int ldl, int ncols, int W,
                                                              const float* __restrict__ cum, float* __restrict__ cand_s,
                                                              float* __restrict__ cand_lp, int* __restrict__ cand_v) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    __shared__ unsigned ck[BEAM_MAX_W];
    __shared__ int cv[BEAM_MAX_W];
    __shared__ int wave_eq[PICK_THREADS / 64];
    __shared__ int n_gt;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (long long)r * ldl;
    auto val = [&](int v) -> float { return STAGED ? srow[v] : row[v]; };

    if (tid == 0) n_gt = 0;            // (ordered before its first use by the sweep's barriers)
    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);
    const int wr = min(W, ncols);
    if (wr == 1 && mx > -INFINITY) {
        // the sweep's column is the best one already: the largest comparable logit, lowest index on ties
        if (tid == 0) { ck[0] = beam_key(mx); cv[0] = mi; }
    } else {
        const unsigned kth = radix_select(sh.rs, ncols, [&](int v) { return beam_key(val(v)); }, [](int) { return 1; }, [&](int) { return wr; });
        const int need_eq = sh.rs.left, n_above = wr - need_eq;
        int eq_base = 0;
        for (int v0 = 0; v0 < ncols; v0 += PICK_THREADS) {
            const int v = v0 + tid;
            const unsigned key = v < ncols ? beam_key(val(v)) : 0u;
            const bool eq = v < ncols && key == kth;
            if (v < ncols && key > kth) {           // fewer than wr of these in the row: slot < n_above
                const int slot = atomicAdd(&n_gt, 1);
                if (slot < BEAM_MAX_W) { ck[slot] = key; cv[slot] = v; }
            }
            const unsigned long long m = __ballot(eq);
            if (lane == 0) wave_eq[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < PICK_THREADS / 64; ++w) {
                const int c = wave_eq[w];
                if (w < wave) before += c;
                total += c;
            }
            const int gt_seen = n_gt;               // (no thread adds to it before the barrier below)
            const int rank = eq_base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (eq && rank < need_eq) { ck[n_above + rank] = key; cv[n_above + rank] = v; }
            eq_base += total;
            __syncthreads();
            if (eq_base >= need_eq && gt_seen == n_above) break;     // uniform: every thread read the same counts
        }
    }
    __syncthreads();
    if (tid < W) {
        if (tid < wr) {
            const unsigned ki = ck[tid];
            const int vi = cv[tid];
            int rank = 0;
            for (int m = 0; m < wr; ++m) rank += (ck[m] > ki || (ck[m] == ki && cv[m] < vi)) ? 1 : 0;
            const float lp = val(vi) - lse;
            const long long o = (long long)r * W + rank;
            cand_v[o] = vi;
            cand_lp[o] = lp;
            cand_s[o] = cum[r] + lp;
        } else {
            cand_v[(long long)r * W + tid] = -1;
        }
    }
}

// One group per workgroup: bitonic sort (descending) of the W x W candidates' 64-bit keys
// [score key:32 | valid:1 | 63 - j:6 | 63 - rank in row:6] in LDS (distinct keys: the order is total), the first W become the
// next slots: parent slot, token, lp, cum, and the token each row reads at the next position.
__global__ __launch_bounds__(SEL_THREADS) void k_beam_select(int W, int ncols, const float* __restrict__ cand_s, const float* __restrict__ cand_lp,
                                                             const int* __restrict__ cand_v, float* __restrict__ cum, int* __restrict__ tok,
                                                             int ldtok, int pos_out, int* __restrict__ par, int* __restrict__ htok,
                                                             float* __restrict__ hlp) {
    __shared__ unsigned long long keys[BEAM_MAX_W * BEAM_MAX_W];
    const int g = blockIdx.x, tid = threadIdx.x, WW = W * W;
    int N = 1;
    while (N < WW) N <<= 1;
    const long long c0 = (long long)g * WW;
    for (int i = tid; i < N; i += SEL_THREADS) {
        unsigned long long k = 0ull;
        if (i < WW && cand_v[c0 + i] >= 0) {
            const int j = i / W, q = i - j * W;
            k = ((unsigned long long)beam_key(cand_s[c0 + i]) << 32) | (1ull << 12) | ((unsigned long long)(63 - j) << 6) |
                (unsigned long long)(63 - q);
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int q = tid; q < (N >> 1); q += SEL_THREADS) {      // pair q: i (bit jj clear) and i + jj
                const int i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1)), ixj = i + jj;
                const unsigned long long a = keys[i], b = keys[ixj];
                if (((i & k) == 0) ? (a < b) : (a > b)) { keys[i] = b; keys[ixj] = a; }
            }
            __syncthreads();
        }
    }
    for (int n = tid; n < W; n += SEL_THREADS) {
        const unsigned long long k = keys[n];
        const int j = 63 - (int)((k >> 6) & 63ull), q = 63 - (int)(k & 63ull);
        // a valid key always names a live candidate (W x min(W, ncols) >= W of them); the guard only keeps the indices in range
        const bool ok = ((k >> 12) & 1ull) && j < W && q < W;
        const long long c = c0 + (ok ? (long long)j * W + q : 0);
        const int r = g * W + n;
        const int v = min(max(cand_v[c], 0), ncols - 1);
        par[r] = ok ? j : 0;
        htok[r] = v;
        hlp[r] = cand_lp[c];
        cum[r] = cand_s[c];
        tok[(long long)r * ldtok + pos_out] = v;
    }
}

// h_dst[l][r] = h_src[l][parent row of r], c likewise (float4 per thread); parent row = (r / W) * W + par[r]
__global__ void k_beam_reorder(int L, int R, int W, int Hp, const int* __restrict__ par, const float* __restrict__ h_src,
                               float* __restrict__ h_dst, const float* __restrict__ c_src, float* __restrict__ c_dst) {
    const int q4 = Hp >> 2;
    const long long n = (long long)L * R * q4;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int u = (int)(i % q4);
        const long long lr = i / q4;
        const int r = (int)(lr % R), l = (int)(lr / R);
        const long long src = ((long long)l * R + (long long)(r / W) * W + par[r]) * Hp + 4 * u, dst = lr * Hp + 4 * u;
        *(float4*)(h_dst + dst) = *(const float4*)(h_src + src);
        *(float4*)(c_dst + dst) = *(const float4*)(c_src + src);
    }
}

// cum[r] = 0 for slot 0 of each group, -inf for the others
__global__ void k_beam_init(float* __restrict__ cum, int R, int W) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) cum[r] = (r % W) == 0 ? 0.0f : -INFINITY;
}

// one thread per final hypothesis (g, n): follow the parents from the last position back -> out_tok / out_lp [r][num], score
__global__ void k_beam_backtrace(int R, int W, int num, const int* __restrict__ par, const int* __restrict__ htok, const float* __restrict__ hlp,
                                 const float* __restrict__ cum, int* __restrict__ out_tok, float* __restrict__ out_lp,
                                 float* __restrict__ out_score) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const int g0 = r - r % W;
    int slot = r - g0;
    out_score[r] = cum[r];
    for (int t = num - 1; t >= 0; --t) {
        const long long e = (long long)t * R + g0 + slot;
        out_tok[(long long)r * num + t] = htok[e];
        out_lp[(long long)r * num + t] = hlp[e];
        slot = par[e];
    }
}

// ---------------------------------------------------------------- the filtered pick (fsmg_generate_filtered, DESIGN.md "Sampling filters")
// k_gen_pick with the sampling filters; one row per workgroup.  lse and out_lp come from the raw row exactly as in k_gen_pick.
// z' = the row with the repetition penalty applied once to each distinct id of tok[b][first .. pos_out - 1] (theta == 1: none).
// T == 0 or top_k == 1: the argmax of z' (lowest column; column 0 when no z' is comparable).  Else k_gen_pick's Gumbel-max over
// z' >= thr, thr the largest of: the top_k-th largest z' (NaN lowest), zmax + T ln(min_p) (min_p > 0), the top-p boundary
// (0 < top_p < 1).  Dynamic LDS: STAGED, the row, its penalised entries rewritten in place from the global raw values
// (idempotent, so repeated ids are harmless); else, with a penalty, a presence bitmap of ceil(ncols / 32) words.
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_gen_pick_filtered(const float* __restrict__ logits, int ldl, int ncols, float temperature,
                                                                    int top_k, float top_p, float min_p, float theta, int window,
                                                                    unsigned seed_lo, unsigned seed_hi, int t, int ctr_t,
                                                                    int* __restrict__ tok, int ldtok, int pos_out,
                                                                    int* __restrict__ out_tok, float* __restrict__ out_lp, int num) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    __shared__ RadixShared<unsigned long long> fs;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (long long)b * ldl;
    const int* trow = tok + (long long)b * ldtok;
    unsigned* bits = (unsigned*)srow;
    const bool pen = theta != 1.0f;
    auto penalise = [&](float z) -> float { return z > 0.0f ? z / theta : z * theta; };
    auto val = [&](int v) -> float {
        if (STAGED) return srow[v];
        const float z = row[v];
        return pen && ((bits[v >> 5] >> (v & 31)) & 1u) ? penalise(z) : z;
    };

    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);

    if (pen) {      // the context tokens in the window (tok[b][0] is the start word, not part of it)
        const int first = window > 0 ? max(1, pos_out - window) : 1;
        if (!STAGED) {
            for (int i = tid; i < (ncols + 31) >> 5; i += PICK_THREADS) bits[i] = 0u;
            __syncthreads();
        }
        for (int i = first + tid; i < pos_out; i += PICK_THREADS) {
            const int v = trow[i];
            if (v < 0 || v >= ncols) continue;
            if (STAGED) srow[v] = penalise(row[v]);
            else atomicOr(&bits[v >> 5], 1u << (v & 31));
        }
        __syncthreads();
    }
    // zmax and its lowest column over the comparable z': the sweep's own (mx, mi) when nothing is penalised and mx > -inf
    float zm = mx; int zi = mi;
    if (pen || !(mx > -INFINITY)) {
        zm = -INFINITY; zi = ncols;
        for (int v = tid; v < ncols; v += PICK_THREADS) {
            const float z = val(v);
            if (z > zm || (z == zm && v < zi)) { zm = z; zi = v; }
        }
        block_argmax(sh, zm, zi);
        if (zi >= ncols) zi = 0;
    }

    int best = zi;
    if (temperature > 0.0f && top_k != 1) {
        float thr = -INFINITY;
        if (top_k > 1 && top_k < ncols) {
            const unsigned kk = radix_select(sh.rs, ncols, [&](int v) { return beam_key(val(v)); }, [](int) { return 1; }, [&](int) { return top_k; });
            if (kk != 0u) thr = key_float(kk);          // (key 0: fewer than top_k comparable columns, all of them stay)
        }
        if (min_p > 0.0f) thr = fmaxf(thr, zm + temperature * logf(min_p));
        if (top_p > 0.0f && top_p < 1.0f) {
            // the top-p boundary over the survivors (z' >= thr): the largest key x with M(>= x) >= ceil(p * Z), M(>= x) the mass of
            // the survivors with key >= x and Z the mass of all of them; a survivor's mass is exp((z' - zmax) / T) in fixed point,
            // 2^32 for z' = zmax
            const float thr1 = thr;
            const unsigned xp = radix_select(
                fs, ncols, [&](int v) { return beam_key(val(v)); },
                [&](int v) -> unsigned long long {
                    const float z = val(v);
                    if (!(z >= thr1)) return 0ull;
                    const float d = z == zm ? 0.0f : (z - zm) / temperature;
                    return (unsigned long long)(expf(d) * 0x1p32f);
                },
                [&](unsigned long long Z) {
                    const double want = ceil((double)top_p * (double)Z);
                    const unsigned long long kl = want < 1.0 ? 1ull : (unsigned long long)want;
                    return kl > Z ? Z : kl;
                });
            if (xp != 0u) thr = key_float(xp);          // a survivor's key, so >= the thresholds above
        }
        best = gumbel_max(sh, ncols, thr, temperature, seed_lo, seed_hi, ctr_t, b, zi, val);
    }
    write_pick(best, row, lse, ncols, b, t, tok, ldtok, pos_out, out_tok, out_lp, num);
}

// ---------------------------------------------------------------- the constrained pick (fsmg_generate_constrained)
// column v in the allowed set of (nline = next[s][*], open)?  (ConstraintDev's comment has the encoding; the masks only keep the
// LDS indices in range -- creation checked the tables)
__device__ __forceinline__ bool con_ok(float bias, unsigned cls, unsigned w, const unsigned* open, const short* nline) {
    const unsigned k = (w & 0x7FFFFFFFu) - 1u;
    const bool slot_ok = w == 0u || ((open[(k >> 5) & (CON_MAX_SLOTS / 32 - 1)] >> (k & 31u)) & 1u) == (w >> 31);
    return bias > -INFINITY && nline[cls & (CON_MAX_CLASSES - 1)] >= 0 && slot_ok;
}
__device__ __forceinline__ bool con_allowed(const ConstraintDev& c, const unsigned* open, const short* nline, int v) {
    return con_ok(c.bias[v], c.cls[v], c.slot[v], open, nline);        // (three independent loads, in flight together)
}

// k_gen_pick_filtered on the constrained logits z^c; one row per workgroup.  lse and out_lp come from the raw row exactly as in
// k_gen_pick.  z^c_v = fl(z_v + bias_v) for v in Omega (the allowed set of the row's state), -inf elsewhere; the penalty, top-k,
// min-p, top-p and the Gumbel-max then run on z^c as they run on z in k_gen_pick_filtered.  One sweep evaluates the predicate (the
// bias, the class byte and the slot word of a column come from global memory, four columns' loads in flight per thread): STAGED, it
// rewrites the staged row to z^c; else it leaves Omega as a bitmap of ceil(ncols / 32) words at the head of the dynamic LDS (the
// penalty's presence bitmap behind it), and val(v) adds the bias on the fly.  The sweep's reduction yields Omega's lowest column,
// ncols when Omega is empty: the dead end, picked from z like
// k_gen_pick_filtered picks it, the state left alone, dead[b] counted up.  A column outside a non-empty Omega is never picked:
// when no allowed column compares above -inf the pick is Omega's lowest column.  Thread 0 advances the state after the pick.
// The row's open bits and its next[s][*] line sit in static LDS (768 B) beside the staged row.
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_gen_pick_constrained(const float* __restrict__ logits, int ldl, int ncols, float temperature,
                                                                       int top_k, float top_p, float min_p, float theta, int window,
                                                                       ConstraintDev c, unsigned seed_lo, unsigned seed_hi, int t, int ctr_t,
                                                                       int* __restrict__ tok, int ldtok, int pos_out,
                                                                       int* __restrict__ out_tok, float* __restrict__ out_lp, int num) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    __shared__ RadixShared<unsigned long long> fs;
    __shared__ unsigned copen[CON_MAX_SLOTS / 32];
    __shared__ short nline[CON_MAX_CLASSES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (long long)b * ldl;
    const int* trow = tok + (long long)b * ldtok;
    const int nw = (ncols + 31) >> 5;
    unsigned* abits = (unsigned*)srow;          // unstaged: Omega, then the penalty's presence bitmap
    unsigned* bits = abits + nw;
    const bool pen = theta != 1.0f;
    bool dead = false;
    auto penalise = [&](float z) -> float { return z > 0.0f ? z / theta : z * theta; };
    auto allowed = [&](int v) -> bool {
        return STAGED ? con_allowed(c, copen, nline, v) : ((abits[v >> 5] >> (v & 31)) & 1u) != 0u;
    };
    auto zc = [&](int v) -> float {       // z^c from the raw row (z itself at a dead end)
        const float z = row[v];
        return dead ? z : allowed(v) ? z + c.bias[v] : -INFINITY;
    };
    auto val = [&](int v) -> float {
        if (STAGED) return srow[v];
        const float z = zc(v);
        return pen && ((bits[v >> 5] >> (v & 31)) & 1u) ? penalise(z) : z;
    };

    // the row's constraint state -> LDS (ordered before its readers by the sweep's barriers)
    const int s0 = min(max(c.state[b], 0), c.S - 1);
    for (int i = tid; i < c.KW && i < CON_MAX_SLOTS / 32; i += PICK_THREADS) copen[i] = c.open[(long long)b * c.KW + i];
    if (tid < CON_MAX_CLASSES) nline[tid] = tid < c.C ? c.next[s0 * c.C + tid] : (short)-1;

    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);

    // Omega's lowest column (and, STAGED, the row rewritten to z^c)
    float any = -INFINITY; int lo = ncols;
    for (int v0 = tid; v0 - tid < ncols; v0 += 4 * PICK_THREADS) {         // (block-uniform trip count: the ballots below)
        float bv[4]; unsigned cw[4], sw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = v0 + j * PICK_THREADS;
            const bool in = v < ncols;
            bv[j] = in ? c.bias[v] : -INFINITY;
            cw[j] = in ? c.cls[v] : 0u;
            sw[j] = in ? c.slot[v] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = v0 + j * PICK_THREADS;
            const bool ok = v < ncols && con_ok(bv[j], cw[j], sw[j], copen, nline);
            if (ok && v < lo) { any = 0.0f; lo = v; }
            if (STAGED) {
                if (v < ncols) srow[v] = ok ? srow[v] + bv[j] : -INFINITY;
            } else {        // a wave's 64 consecutive columns are two words of the bitmap (v - lane is a multiple of 64)
                const unsigned long long mk = __ballot(ok);
                const int wi = (v - (tid & 63)) >> 5;
                if ((tid & 63) == 0 && wi < nw) {
                    abits[wi] = (unsigned)mk;
                    if (wi + 1 < nw) abits[wi + 1] = (unsigned)(mk >> 32);
                }
            }
        }
    }
    block_argmax(sh, any, lo);
    dead = !(any > -INFINITY);
    if (dead && STAGED) {       // nothing is allowed: back to z
        for (int v = tid; v < ncols; v += PICK_THREADS) srow[v] = row[v];
    }
    __syncthreads();

    if (pen) {      // the context tokens in the window (tok[b][0] is the start word, not part of it)
        const int first = window > 0 ? max(1, pos_out - window) : 1;
        if (!STAGED) {
            for (int i = tid; i < (ncols + 31) >> 5; i += PICK_THREADS) bits[i] = 0u;
            __syncthreads();
        }
        for (int i = first + tid; i < pos_out; i += PICK_THREADS) {
            const int v = trow[i];
            if (v < 0 || v >= ncols) continue;
            if (STAGED) srow[v] = penalise(zc(v));
            else atomicOr(&bits[v >> 5], 1u << (v & 31));
        }
        __syncthreads();
    }
    // zmax and its lowest column over the comparable values; flat: none compares above -inf
    float zm = -INFINITY; int zi = ncols;
    for (int v = tid; v < ncols; v += PICK_THREADS) {
        const float z = val(v);
        if (z > zm || (z == zm && v < zi)) { zm = z; zi = v; }
    }
    block_argmax(sh, zm, zi);
    const bool flat = !(zm > -INFINITY);
    if (zi >= ncols) zi = 0;
    if (flat && !dead) zi = lo;

    int best = zi;
    if (temperature > 0.0f && top_k != 1 && (dead || !flat)) {
        float thr = -INFINITY;
        if (top_k > 1 && top_k < ncols) {
            const unsigned kk = radix_select(sh.rs, ncols, [&](int v) { return beam_key(val(v)); }, [](int) { return 1; }, [&](int) { return top_k; });
            if (kk != 0u) thr = key_float(kk);
        }
        if (min_p > 0.0f) thr = fmaxf(thr, zm + temperature * logf(min_p));
        if (top_p > 0.0f && top_p < 1.0f) {       // k_gen_pick_filtered's top-p boundary, on z^c
            const float thr1 = thr;
            const unsigned xp = radix_select(
                fs, ncols, [&](int v) { return beam_key(val(v)); },
                [&](int v) -> unsigned long long {
                    const float z = val(v);
                    if (!(z >= thr1)) return 0ull;
                    const float d = z == zm ? 0.0f : (z - zm) / temperature;
                    return (unsigned long long)(expf(d) * 0x1p32f);
                },
                [&](unsigned long long Z) {
                    const double want = ceil((double)top_p * (double)Z);
                    const unsigned long long kl = want < 1.0 ? 1ull : (unsigned long long)want;
                    return kl > Z ? Z : kl;
                });
            if (xp != 0u) thr = key_float(xp);
        }
        best = gumbel_max(sh, ncols, thr, temperature, seed_lo, seed_hi, ctr_t, b, zi, val);
    }
    best = min(max(best, 0), ncols - 1);
    write_pick(best, row, lse, ncols, b, t, tok, ldtok, pos_out, out_tok, out_lp, num);
    if (tid == 0) {
        if (dead) {
            c.dead[b] += 1;
        } else {
            c.state[b] = nline[c.cls[best] & (CON_MAX_CLASSES - 1)];
            const unsigned w = c.slot[best];
            if (w != 0u) {
                const unsigned k = (w & 0x7FFFFFFFu) - 1u, wi = (k >> 5) & (CON_MAX_SLOTS / 32 - 1);
                if ((int)wi < c.KW) c.open[(long long)b * c.KW + wi] = copen[wi] ^ (1u << (k & 31u));
            }
        }
    }
}

// One thread per row: the row's state walked over its primer tokens tok[b][1 .. P] in order (the start word at tok[b][0] advances
// nothing).  A token that is not allowed where it stands raises *err and is stepped over.
__global__ void k_constraint_advance(ConstraintDev c, int ncols, int B, int P, const int* __restrict__ tok, int ldtok, int* __restrict__ err) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    unsigned* open = c.open + (long long)b * c.KW;
    int s = c.state[b];
    bool bad = s < 0 || s >= c.S;
    if (bad) s = 0;
    for (int p = 1; p <= P; ++p) {
        const int v = tok[(long long)b * ldtok + p];
        if (v < 0 || v >= ncols) { bad = true; continue; }
        const int nx = c.next[s * c.C + (c.cls[v] & (CON_MAX_CLASSES - 1))];
        const unsigned w = c.slot[v];
        const unsigned k = (w & 0x7FFFFFFFu) - 1u;
        bool ok = c.bias[v] > -INFINITY && nx >= 0;
        unsigned word = 0u;
        if (w != 0u) {
            if ((int)(k >> 5) >= c.KW) { bad = true; continue; }
            word = open[k >> 5];
            ok = ok && ((word >> (k & 31u)) & 1u) == (w >> 31);
        }
        if (!ok) { bad = true; continue; }
        s = nx;
        if (w != 0u) open[k >> 5] = word ^ (1u << (k & 31u));
    }
    c.state[b] = s;
    if (bad) atomicOr(err, 1);
}

// ---------------------------------------------------------------- constrained beam search (fsmg_beam_search_constrained)
// Every row r = g * W + j carries a constraint state (c.state[r], c.open[r], c.dead[r]).  Per generated position:
// k_beam_rowtop_constrained (the row's best candidates over Omega only), k_beam_select_constrained (the tiered ranking; the new
// slots' state and dead ends), k_beam_con_reorder (the new slots' open bits).  The state arrays are double-buffered like h / c: a
// new slot reads its parent's row of the old buffer.

// block-wide integer sum -- every thread gets the result (integers: the tree's shape cannot change it)
__device__ __forceinline__ int block_isum(PickShared& sh, int s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.iv[w] = s;
    __syncthreads();
    int t = 0;
    for (int k = 0; k < PICK_THREADS / 64; ++k) t += sh.iv[k];
    return t;
}

// a staged row's excluded columns hold this NaN; an allowed column's NaN is stored as the quiet NaN below, so the two never meet
constexpr unsigned CON_EXCLUDED = 0xFFFFFFFFu, CON_QNAN = 0x7FC00000u;

// k_beam_rowtop under a constraint; one row per workgroup.  lse comes from the raw row (row_max_lse, the number k_beam_rowtop
// uses).  The Omega sweep of k_gen_pick_constrained follows (four columns' bias, class and slot loads in flight): STAGED, it rewrites
// the row to z^c = fl(z + bias) over Omega and marks the other columns CON_EXCLUDED; else it leaves Omega as a bitmap of
// ceil(ncols / 32) words in the dynamic LDS and val(v) adds the bias on the fly.  The sweep also counts |Omega|.  The row's
// candidates are its min(W, |Omega|) best columns of Omega by (z^c descending, NaN lowest, v ascending): an excluded column weighs
// nothing in the radix select and is skipped by the gather, so it ranks below an allowed NaN.  lp = fl(z^c - lse), s = fl(cum + lp);
// cand_v = -1 pads a short row.  Dead end (Omega empty): k_beam_rowtop's body on z over all columns, row_dead[r] = 1.
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_beam_rowtop_constrained(const float* __restrict__ logits, int ldl, int ncols, int W,
                                                                          const float* __restrict__ cum, ConstraintDev c,
                                                                          float* __restrict__ cand_s, float* __restrict__ cand_lp,
                                                                          int* __restrict__ cand_v, int* __restrict__ row_dead) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    __shared__ unsigned ck[BEAM_MAX_W];
    __shared__ int cv[BEAM_MAX_W];
    __shared__ int wave_eq[PICK_THREADS / 64];
    __shared__ int n_gt;
    __shared__ unsigned copen[CON_MAX_SLOTS / 32];
    __shared__ short nline[CON_MAX_CLASSES];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = logits + (long long)r * ldl;
    const int nw = (ncols + 31) >> 5;
    unsigned* abits = (unsigned*)srow;          // unstaged: Omega
    bool dead = false;
    auto in_set = [&](int v) -> bool {
        if (dead) return true;
        return STAGED ? __float_as_uint(srow[v]) != CON_EXCLUDED : ((abits[v >> 5] >> (v & 31)) & 1u) != 0u;
    };
    auto val = [&](int v) -> float {            // z^c of a column of the set (z itself at a dead end)
        if (STAGED) return srow[v];
        const float z = row[v];
        return dead ? z : z + c.bias[v];
    };

    if (tid == 0) n_gt = 0;            // (ordered before its first use by the sweep's barriers)
    // the row's constraint state -> LDS (ordered before its readers by the sweep's barriers)
    const int s0 = min(max(c.state[r], 0), c.S - 1);
    for (int i = tid; i < c.KW && i < CON_MAX_SLOTS / 32; i += PICK_THREADS) copen[i] = c.open[(long long)r * c.KW + i];
    if (tid < CON_MAX_CLASSES) nline[tid] = tid < c.C ? c.next[s0 * c.C + tid] : (short)-1;

    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);

    int cnt = 0;
    for (int v0 = tid; v0 - tid < ncols; v0 += 4 * PICK_THREADS) {         // (block-uniform trip count: the ballots below)
        float bv[4]; unsigned cw[4], sw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = v0 + j * PICK_THREADS;
            const bool in = v < ncols;
            bv[j] = in ? c.bias[v] : -INFINITY;
            cw[j] = in ? c.cls[v] : 0u;
            sw[j] = in ? c.slot[v] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = v0 + j * PICK_THREADS;
            const bool ok = v < ncols && con_ok(bv[j], cw[j], sw[j], copen, nline);
            cnt += ok ? 1 : 0;
            if (STAGED) {
                if (v < ncols) {
                    const float zc = srow[v] + bv[j];
                    srow[v] = __uint_as_float(!ok ? CON_EXCLUDED : zc != zc ? CON_QNAN : __float_as_uint(zc));
                }
            } else {        // a wave's 64 consecutive columns are two words of the bitmap (v - lane is a multiple of 64)
                const unsigned long long mk = __ballot(ok);
                const int wi = (v - lane) >> 5;
                if (lane == 0 && wi < nw) {
                    abits[wi] = (unsigned)mk;
                    if (wi + 1 < nw) abits[wi + 1] = (unsigned)(mk >> 32);
                }
            }
        }
    }
    const int n_om = block_isum(sh, cnt);       // (its barriers order the sweep's LDS stores before the reads below)
    dead = n_om == 0;
    if (dead && STAGED) {       // nothing is allowed: back to z
        for (int v = tid; v < ncols; v += PICK_THREADS) srow[v] = row[v];
        __syncthreads();
    }

    const int wr = dead ? min(W, ncols) : min(W, n_om);
    const unsigned kth = radix_select(sh.rs, ncols, [&](int v) { return beam_key(val(v)); }, [&](int v) { return in_set(v) ? 1 : 0; },
                                      [&](int) { return wr; });
    const int need_eq = sh.rs.left, n_above = wr - need_eq;
    int eq_base = 0;
    for (int v0 = 0; v0 < ncols; v0 += PICK_THREADS) {
        const int v = v0 + tid;
        const bool in = v < ncols && in_set(v);
        const unsigned key = in ? beam_key(val(v)) : 0u;
        const bool eq = in && key == kth;
        if (in && key > kth) {                  // fewer than wr of these in the row: slot < n_above
            const int slot = atomicAdd(&n_gt, 1);
            if (slot < BEAM_MAX_W) { ck[slot] = key; cv[slot] = v; }
        }
        const unsigned long long m = __ballot(eq);
        if (lane == 0) wave_eq[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < PICK_THREADS / 64; ++w) {
            const int n = wave_eq[w];
            if (w < wave) before += n;
            total += n;
        }
        const int gt_seen = n_gt;               // (no thread adds to it before the barrier below)
        const int rank = eq_base + before + __popcll(m & ((1ull << lane) - 1ull));
        if (eq && rank < need_eq && n_above + rank < BEAM_MAX_W) { ck[n_above + rank] = key; cv[n_above + rank] = v; }
        eq_base += total;
        __syncthreads();
        if (eq_base >= need_eq && gt_seen == n_above) break;     // uniform: every thread read the same counts
    }
    __syncthreads();
    if (tid == 0) row_dead[r] = dead ? 1 : 0;
    if (tid < W) {
        if (tid < wr) {
            const unsigned ki = ck[tid];
            const int vi = min(max(cv[tid], 0), ncols - 1);
            int rank = 0;
            for (int m = 0; m < wr; ++m) rank += (ck[m] > ki || (ck[m] == ki && cv[m] < vi)) ? 1 : 0;
            const float lp = val(vi) - lse;
            const long long o = (long long)r * W + rank;
            cand_v[o] = vi;
            cand_lp[o] = lp;
            cand_s[o] = cum[r] + lp;
        } else {
            cand_v[(long long)r * W + tid] = -1;
        }
    }
}

// k_beam_select with the tier above the score: the 64-bit key is [live row:1 | score key:32 | valid:1 | 63 - j:6 | 63 - rank in
// row:6], so every candidate of a row that is not at a dead end ranks above every candidate of one that is.  The winners' loop also
// gives each new slot its parent's state advanced by the token (a dead-end parent: the state unchanged, one more dead end), read
// from the old buffer `c` and written to state_new / dead_new.
__global__ __launch_bounds__(SEL_THREADS) void k_beam_select_constrained(int W, int ncols, const float* __restrict__ cand_s,
                                                                         const float* __restrict__ cand_lp, const int* __restrict__ cand_v,
                                                                         const int* __restrict__ row_dead, ConstraintDev c,
                                                                         int* __restrict__ state_new, int* __restrict__ dead_new,
                                                                         float* __restrict__ cum, int* __restrict__ tok, int ldtok, int pos_out,
                                                                         int* __restrict__ par, int* __restrict__ htok, float* __restrict__ hlp) {
    __shared__ unsigned long long keys[BEAM_MAX_W * BEAM_MAX_W];
    const int g = blockIdx.x, tid = threadIdx.x, WW = W * W;
    int N = 1;
    while (N < WW) N <<= 1;
    const long long c0 = (long long)g * WW;
    for (int i = tid; i < N; i += SEL_THREADS) {
        unsigned long long k = 0ull;
        if (i < WW && cand_v[c0 + i] >= 0) {
            const int j = i / W, q = i - j * W;
            k = ((unsigned long long)(row_dead[g * W + j] ? 0 : 1) << 45) | ((unsigned long long)beam_key(cand_s[c0 + i]) << 13) | (1ull << 12) |
                ((unsigned long long)(63 - j) << 6) | (unsigned long long)(63 - q);
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int jj = k >> 1; jj > 0; jj >>= 1) {
            for (int q = tid; q < (N >> 1); q += SEL_THREADS) {      // pair q: i (bit jj clear) and i + jj
                const int i = ((q & ~(jj - 1)) << 1) | (q & (jj - 1)), ixj = i + jj;
                const unsigned long long a = keys[i], b = keys[ixj];
                if (((i & k) == 0) ? (a < b) : (a > b)) { keys[i] = b; keys[ixj] = a; }
            }
            __syncthreads();
        }
    }
    for (int n = tid; n < W; n += SEL_THREADS) {
        const unsigned long long k = keys[n];
        const int j = 63 - (int)((k >> 6) & 63ull), q = 63 - (int)(k & 63ull);
        // a valid key always names a live candidate (every row has at least one); the guard only keeps the indices in range
        const bool ok = ((k >> 12) & 1ull) && j < W && q < W;
        const long long cd = c0 + (ok ? (long long)j * W + q : 0);
        const int r = g * W + n, rp = g * W + (ok ? j : 0);
        const int v = min(max(cand_v[cd], 0), ncols - 1);
        par[r] = ok ? j : 0;
        htok[r] = v;
        hlp[r] = cand_lp[cd];
        cum[r] = cand_s[cd];
        tok[(long long)r * ldtok + pos_out] = v;
        const bool pd = row_dead[rp] != 0;
        const int s0 = min(max(c.state[rp], 0), c.S - 1);
        int nx = pd ? s0 : (int)c.next[s0 * c.C + min((int)c.cls[v], c.C - 1)];
        if (nx < 0 || nx >= c.S) nx = s0;           // (the token lies in Omega: never taken)
        state_new[r] = nx;
        dead_new[r] = c.dead[rp] + (pd ? 1 : 0);
    }
}

// open_dst[r] = open_src[parent row of r] with the chosen token's slot bit flipped (a dead-end parent: unchanged); one thread per
// word.  parent row = (r / W) * W + par[r], the token htok[r].
__global__ void k_beam_con_reorder(int R, int W, int KW, const int* __restrict__ par, const int* __restrict__ htok,
                                   const int* __restrict__ row_dead, const unsigned* __restrict__ slot, const unsigned* __restrict__ open_src,
                                   unsigned* __restrict__ open_dst) {
    const long long n = (long long)R * KW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / KW), wi = (int)(i % KW);
        const int rp = (r / W) * W + par[r];
        unsigned word = open_src[(long long)rp * KW + wi];
        if (!row_dead[rp]) {
            const unsigned w = slot[htok[r]];
            const unsigned k = (w & 0x7FFFFFFFu) - 1u;
            if (w != 0u && (int)(k >> 5) == wi) word ^= 1u << (k & 31u);
        }
        open_dst[i] = word;
    }
}

// ---------------------------------------------------------------- decode states (fsmg_dstate_*, DESIGN.md "Decode states")
// The teacher-forced log-prob of fsmg_dstate_feed; one row per workgroup.  lse is the picks' (row_max_lse), so that the log-prob feed
// returns for a token is bitwise the number a pick that chose it reports: out_lp[b][i] = logit[target] - lse, the target the token
// the row reads next, tok[b][pos_tgt] (clamped into [0, ncols): it indexes the row).
template <bool STAGED>
__global__ __launch_bounds__(PICK_THREADS) void k_feed_logprob(const float* __restrict__ logits, int ldl, int ncols,
                                                               const int* __restrict__ tok, int ldtok, int pos_tgt,
                                                               float* __restrict__ out_lp, int n, int i) {
    extern __shared__ float srow[];
    __shared__ PickShared sh;
    const int b = blockIdx.x;
    const float* row = logits + (long long)b * ldl;
    float mx; int mi;
    const float lse = row_max_lse<STAGED>(sh, row, srow, ncols, mx, mi);
    if (threadIdx.x == 0) {
        const int y = min(max(tok[(long long)b * ldtok + pos_tgt], 0), ncols - 1);
        out_lp[(long long)b * n + i] = row[y] - lse;
    }
}

// Rows of a decode state: dst row i takes src row (rows != nullptr ? rows[i] : i / div), h and c of every layer ([L][R][Hp], float4
// per thread) and ntok tokens, tok_src[row][off_src ..] -> tok_dst[i][off_dst ..].  The load of a stateful call (div = W for beam
// search), its commit (div = 1) and fsmg_dstate_gather (rows) are this kernel.  A row index outside [0, Rs) copies nothing.
__global__ void k_dstate_rows(int L, int Rd, int Rs, int Hp, const int* __restrict__ rows, int div, const float* __restrict__ h_src,
                              float* __restrict__ h_dst, const float* __restrict__ c_src, float* __restrict__ c_dst,
                              const int* __restrict__ tok_src, int ld_src, int off_src, int* __restrict__ tok_dst, int ld_dst, int off_dst,
                              int ntok) {
    const int q4 = Hp >> 2;
    const long long n_state = (long long)L * Rd * q4, n = n_state + (long long)Rd * ntok;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (i < n_state) {
            const int u = (int)(i % q4);
            const long long lr = i / q4;
            const int r = (int)(lr % Rd), l = (int)(lr / Rd);
            const int sr = rows != nullptr ? rows[r] : r / div;
            if (sr < 0 || sr >= Rs) continue;
            const long long src = ((long long)l * Rs + sr) * Hp + 4 * u, dst = lr * Hp + 4 * u;
            *(float4*)(h_dst + dst) = *(const float4*)(h_src + src);
            *(float4*)(c_dst + dst) = *(const float4*)(c_src + src);
        } else {
            const long long j = i - n_state;
            const int r = (int)(j / ntok), p = (int)(j % ntok);
            const int sr = rows != nullptr ? rows[r] : r / div;
            if (sr < 0 || sr >= Rs) continue;
            tok_dst[(long long)r * ld_dst + off_dst + p] = tok_src[(long long)sr * ld_src + off_src + p];
        }
    }
}

// a fresh state: zero h and c ([L][R][Hp]), every token slot the start word
__global__ void k_dstate_reset(long long n_state, float* __restrict__ hh, float* __restrict__ cc, long long n_tok, int* __restrict__ tok,
                               int start) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n_state + n_tok; i += (long long)gridDim.x * blockDim.x) {
        if (i < n_state) { hh[i] = 0.0f; cc[i] = 0.0f; }
        else tok[i - n_state] = start;
    }
}

// the fed tokens of a call, tokens [R][n] -> tok[r][off + i]; *err = 1 for an id outside [0, ncols) (the start word is allowed), which
// is stored as the start word: the cells gather an embedding row by it
__global__ void k_dstate_tokens(const int* __restrict__ tokens, int R, int n, int ncols, int start, int* __restrict__ tok, int ldtok, int off,
                                int* __restrict__ err) {
    const long long total = (long long)R * n;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / n), p = (int)(i % n);
        int w = tokens[i];
        if (w < 0 || w >= ncols) { atomicOr(err, 1); w = start; }
        tok[(long long)r * ldtok + off + p] = w;
    }
}

// ---------------------------------------------------------------- cache-conditioned generation, stage two (fsmg_kernels.h)
// block-wide maximum of doubles -- every thread gets the result (a maximum: the tree's shape cannot change it)
__device__ __forceinline__ double block_max(PickShared& sh, double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.dv[w] = v;
    __syncthreads();
    double t = sh.dv[0];
    for (int k = 1; k < PICK_THREADS / 64; ++k) t = fmax(t, sh.dv[k]);
    return t;
}

// The three pieces k_cache_mix and k_cache_mix_self share (CacheMixArgs' comment has the steps).
// w_i = ca_exp2(u d_i - S) written over the n scores at d; this thread's share of their sum goes on top of z
__device__ __forceinline__ void mix_weights(double* d, int n, double u, double S, double& z) {
    for (int i = threadIdx.x; i < n; i += PICK_THREADS) {
        const double w = ca_exp2(fma(u, d[i], -S));
        d[i] = w;
        z += w;
    }
}

// The distinct values of group g through the value index: the long segments one wave each (lanes stride the segment, then a
// butterfly), the short ones one thread each; put(&value, mass) once per segment, by one thread (the value is loaded where it is
// used, behind the mass's arithmetic).
template <class Put>
__device__ __forceinline__ void mix_walk(const CacheMixArgs& a, int g, const double* d, Put&& put) {
    const int tid = threadIdx.x, Mg = a.Mg;
    const int* order = a.order + (long long)g * Mg;
    const int* seg_beg = a.seg_beg + (long long)g * Mg;
    const int* seg_end = a.seg_end + (long long)g * Mg;
    const int* seg_val = a.seg_val + (long long)g * Mg;
    const int n_seg = a.n_seg[g], n_long = a.n_long[g], lane = tid & 63;
    for (int sg = tid >> 6; sg < n_long; sg += PICK_THREADS / 64) {
        const int j1 = seg_end[sg];
        double mass = 0.0;
        for (int j = seg_beg[sg] + lane; j < j1; j += 64) mass += d[order[j]];
        for (int o = 32; o > 0; o >>= 1) mass += __shfl_xor(mass, o);
        if (lane == 0) put(seg_val + sg, mass);
    }
    for (int sg = n_long + tid; sg < n_seg; sg += PICK_THREADS) {
        const int j1 = seg_end[sg];
        double mass = 0.0;
        for (int j = seg_beg[sg]; j < j1; ++j) mass += d[order[j]];
        put(seg_val + sg, mass);
    }
}

// column v of the output row from the model's log-prob and the cache's probability
__device__ __forceinline__ float mix_column(const CacheMixArgs& a, float lp, float p) {
    if (!a.mix) return lp;
    return p == 0.0f ? (float)(a.log1m_lambda + (double)lp) : mix_logprob(lp, p, a.log1m_lambda, a.log_lambda);
}

// One row per workgroup.  The barriers inside the block reductions order a step's global stores (the masses over D, the pc row)
// before the next step's loads: a workgroup reads back only what it wrote itself.
__global__ __launch_bounds__(PICK_THREADS) void k_cache_mix(CacheMixArgs a) {
    __shared__ PickShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, Mg = a.Mg, ncols = a.ncols;
    float* row = a.logits + (long long)b * a.ldl;
    float* pc = a.pc + (long long)b * a.ldl;
    double* d = a.D + (long long)b * Mg;
    const int g = a.row_group[b];
    const int ng = a.count ? a.count[g] : Mg;       // the row's group's entries (block-uniform); Mg stays the stride of D

    float mx; int mi;
    const float lse = row_max_lse<false>(sh, row, nullptr, ncols, mx, mi);

    double m = -INFINITY;
    for (int i = tid; i < ng; i += PICK_THREADS) m = fmax(m, d[i]);
    m = block_max(sh, m);
    double z = 0.0;
    mix_weights(d, ng, a.u, ceil(a.u * m), z);
    for (int v = tid; v < ncols; v += PICK_THREADS) pc[v] = 0.0f;
    const double Z = block_sum(sh, z);

    mix_walk(a, g, d, [&](const int* v, double mass) { pc[*v] = mass == 0.0 ? 0.0f : (float)(mass / Z); });
    __syncthreads();

    for (int v = tid; v < ncols; v += PICK_THREADS) row[v] = mix_column(a, row[v] - lse, pc[v]);
    if (tid == 0 && a.out_lse) a.out_lse[b] = lse;
}

// k_cache_mix over the union of the support entries and the row's visible own entries (CacheMixSelfArgs' comment)
__global__ __launch_bounds__(PICK_THREADS) void k_cache_mix_self(CacheMixSelfArgs s) {
    __shared__ PickShared sh;
    const CacheMixArgs& a = s.m;
    const int b = blockIdx.x, tid = threadIdx.x, Mg = a.Mg, ncols = a.ncols;
    float* row = a.logits + (long long)b * a.ldl;
    float* pc = a.pc + (long long)b * a.ldl;
    double* pm = s.pm + (long long)b * a.ldl;
    double* d = Mg > 0 ? a.D + (long long)b * Mg : nullptr;
    double* d2 = s.D2 + (long long)b * s.ldo;
    const int len = s.row_len ? s.row_len[b] : s.len;
    const int n = min(len, s.W), lo = len - n;
    const int* val = s.val + (long long)b * s.ldv + lo;
    const int ng = Mg > 0 && a.count ? a.count[a.row_group[b]] : Mg;       // the row's group's entries (block-uniform)

    float mx; int mi;
    const float lse = row_max_lse<false>(sh, row, nullptr, ncols, mx, mi);

    double m = -INFINITY;
    for (int i = tid; i < ng; i += PICK_THREADS) m = fmax(m, d[i]);
    for (int i = tid; i < n; i += PICK_THREADS) m = fmax(m, d2[i]);
    m = block_max(sh, m);
    if (Mg == 0 && n == 0) {                        // the empty union: the model alone (block-uniform)
        for (int v = tid; v < ncols; v += PICK_THREADS) { pc[v] = 0.0f; row[v] = row[v] - lse; }
        if (tid == 0 && a.out_lse) a.out_lse[b] = lse;
        return;
    }
    const double S = ceil(a.u * m);
    double z = 0.0;
    mix_weights(d, ng, a.u, S, z);
    mix_weights(d2, n, a.u, S, z);
    for (int v = tid; v < ncols; v += PICK_THREADS) pm[v] = 0.0;
    const double Z = block_sum(sh, z);

    if (Mg > 0) mix_walk(a, a.row_group[b], d, [&](const int* v, double mass) { pm[*v] = mass; });     // the masses kept in fp64
    __syncthreads();
    // the own entries: the first visible occurrence of a value owns its column and sums its later duplicates in entry order
    for (int j = tid; j < n; j += PICK_THREADS) {
        const int v = val[j];
        bool first = v >= 0 && v < ncols;
        for (int i = 0; i < j && first; ++i) first = val[i] != v;
        if (!first) continue;
        double mass = d2[j];
        for (int i = j + 1; i < n; ++i)
            if (val[i] == v) mass += d2[i];
        pm[v] += mass;
    }
    __syncthreads();

    for (int v = tid; v < ncols; v += PICK_THREADS) {
        const double mass = pm[v];
        const float p = mass == 0.0 ? 0.0f : (float)(mass / Z);
        pc[v] = p;
        row[v] = mix_column(a, row[v] - lse, p);
    }
    if (tid == 0 && a.out_lse) a.out_lse[b] = lse;
}

}  // namespace

hipError_t launch_cache_mix_self(hipStream_t s, int R, const CacheMixSelfArgs& a) {
    if (R <= 0) return hipSuccess;
    if (a.m.ncols <= 0 || a.m.ncols > a.m.ldl || a.m.Mg < 0 || a.W < 1 || a.ldo < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cache_mix_self, dim3(R), dim3(PICK_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_cache_mix(hipStream_t s, int R, const CacheMixArgs& a) {
    if (R <= 0) return hipSuccess;
    if (a.ncols <= 0 || a.ncols > a.ldl || a.Mg < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cache_mix, dim3(R), dim3(PICK_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gen_cell(hipStream_t s, const float* Kx, int in_dim, const float* Kh, const float* bias, int Hp, const float* emb, int ldemb,
                           const int* tok, int ldtok, int pos, const float* x, const float* h_in, float* h_out, float* c, int B) {
    if (B <= 0) return hipSuccess;
    if ((in_dim & 15) || (Hp & 15) || B > 65535 * GEN_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gen_cell, dim3(Hp / 4, (B + GEN_ROWS - 1) / GEN_ROWS), dim3(GEN_THREADS), 0, s, Kx, in_dim, Kh, bias, Hp, emb, ldemb,
                       tok, ldtok, pos, x, h_in, h_out, c, B);
    return hipGetLastError();
}

hipError_t launch_gen_logits(hipStream_t s, const float* W, int ldw, const float* bias, int ncols, const float* h, int Hp, int B,
                             float* logits, int ldl) {
    if (B <= 0) return hipSuccess;
    if ((Hp & 15) || ncols > ldw || ncols > ldl || B > 65535 * GEN_ROWS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gen_logits, dim3((ncols + 15) / 16, (B + GEN_ROWS - 1) / GEN_ROWS), dim3(GEN_THREADS), 0, s, W, ldw, bias, ncols, h, Hp,
                       B, logits, ldl);
    return hipGetLastError();
}

namespace {
// The row-per-workgroup kernels (the picks, k_beam_rowtop), one workgroup per row: the STAGED instantiation holds the row in dynamic
// LDS up to PICK_LDS_FLOATS columns (128 KiB of the 160 KiB), the other reads it from global memory with `lds` bytes of dynamic LDS.
// Both instantiations' LDS limit is raised once per device (a second caller racing the first sets the same value again, harmless).
template <auto* STAGED, auto* UNSTAGED, class... Args>
hipError_t launch_row_kernel(hipStream_t s, int rows, int ncols, size_t lds, Args... args) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        for (const void* k : {(const void*)STAGED, (const void*)UNSTAGED}) {
            e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(float) * PICK_LDS_FLOATS);
            if (e != hipSuccess) return e;
        }
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    if (ncols <= PICK_LDS_FLOATS)
        hipLaunchKernelGGL(STAGED, dim3(rows), dim3(PICK_THREADS), sizeof(float) * (size_t)ncols, s, args...);
    else
        hipLaunchKernelGGL(UNSTAGED, dim3(rows), dim3(PICK_THREADS), lds, s, args...);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_gen_pick(hipStream_t s, const float* logits, int ldl, int ncols, int B, float temperature, int top_k, const GenFilters* f,
                           uint64_t seed, int t, int ctr_t, int* tok, int ldtok, int pos_out, int* out_tok, float* out_lp, int num) {
    if (B <= 0) return hipSuccess;
    if (ncols <= 0 || ncols > ldl || t < 0 || t >= num || ctr_t < t || pos_out >= ldtok || (f && f->window < 0)) return hipErrorInvalidValue;
    const unsigned lo = (unsigned)(seed & 0xFFFFFFFFull), hi = (unsigned)(seed >> 32);
    if (!f)
        return launch_row_kernel<k_gen_pick<true>, k_gen_pick<false>>(s, B, ncols, 0, logits, ldl, ncols, temperature, top_k, lo, hi, t, ctr_t,
                                                                      tok, ldtok, pos_out, out_tok, out_lp, num);
    // an unstaged row with a penalty keeps a presence bitmap of its columns in LDS
    const size_t bitmap_bytes = f->theta != 1.0f ? sizeof(unsigned) * (size_t)((ncols + 31) / 32) : 0;
    if (bitmap_bytes > sizeof(float) * PICK_LDS_FLOATS) return hipErrorInvalidValue;
    return launch_row_kernel<k_gen_pick_filtered<true>, k_gen_pick_filtered<false>>(s, B, ncols, bitmap_bytes, logits, ldl, ncols, temperature,
                                                                                    top_k, f->top_p, f->min_p, f->theta, f->window, lo, hi, t,
                                                                                    ctr_t, tok, ldtok, pos_out, out_tok, out_lp, num);
}

hipError_t launch_gen_pick_constrained(hipStream_t s, const float* logits, int ldl, int ncols, int B, float temperature, int top_k,
                                       const GenFilters* f, const ConstraintDev& c, uint64_t seed, int t, int ctr_t, int* tok, int ldtok,
                                       int pos_out, int* out_tok, float* out_lp, int num) {
    if (B <= 0) return hipSuccess;
    if (ncols <= 0 || ncols > ldl || t < 0 || t >= num || ctr_t < t || pos_out >= ldtok || (f && f->window < 0)) return hipErrorInvalidValue;
    if (c.S < 1 || c.S > CON_MAX_STATES || c.C < 1 || c.C > CON_MAX_CLASSES || c.KW < 0 || c.KW > CON_MAX_SLOTS / 32 || !c.bias || !c.cls ||
        !c.slot || !c.next || !c.state || !c.open || !c.dead)
        return hipErrorInvalidValue;
    const unsigned lo = (unsigned)(seed & 0xFFFFFFFFull), hi = (unsigned)(seed >> 32);
    const GenFilters none{0.0f, 0.0f, 1.0f, 0};
    if (!f) f = &none;
    // an unstaged row keeps Omega as a bitmap of its columns in LDS, and with a penalty the presence bitmap behind it
    const size_t bitmap_bytes = sizeof(unsigned) * (size_t)((ncols + 31) / 32) * (f->theta != 1.0f ? 2 : 1);
    if (bitmap_bytes > sizeof(float) * PICK_LDS_FLOATS) return hipErrorInvalidValue;
    return launch_row_kernel<k_gen_pick_constrained<true>, k_gen_pick_constrained<false>>(s, B, ncols, bitmap_bytes, logits, ldl, ncols,
                                                                                          temperature, top_k, f->top_p, f->min_p, f->theta,
                                                                                          f->window, c, lo, hi, t, ctr_t, tok, ldtok, pos_out,
                                                                                          out_tok, out_lp, num);
}

hipError_t launch_constraint_advance(hipStream_t s, const ConstraintDev& c, int ncols, int B, int P, const int* tok, int ldtok, int* err) {
    if (B <= 0) return hipSuccess;
    if (P < 0 || P + 1 > ldtok || ncols <= 0 || c.S < 1 || c.C < 1 || c.KW < 0 || !tok || !err) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_constraint_advance, dim3((B + 63) / 64), dim3(64), 0, s, c, ncols, B, P, tok, ldtok, err);
    return hipGetLastError();
}

hipError_t launch_gen_primer(hipStream_t s, const int* primer, int B, int P, int vocab, int start, int* tok, int ldtok, int* err,
                             int rows_per_primer) {
    if (B <= 0) return hipSuccess;
    if (P + 1 > ldtok || (P > 0 && primer == nullptr) || rows_per_primer < 1) return hipErrorInvalidValue;
    const long long n = (long long)B * (P + 1);
    const int blocks = (int)std::min<long long>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_gen_primer, dim3(blocks), dim3(256), 0, s, primer, B, P, vocab, start, tok, ldtok, err,
                       rows_per_primer);
    return hipGetLastError();
}

hipError_t launch_beam_init(hipStream_t s, float* cum, int R, int W) {
    if (R <= 0) return hipSuccess;
    if (W < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_beam_init, dim3((R + 255) / 256), dim3(256), 0, s, cum, R, W);
    return hipGetLastError();
}

hipError_t launch_beam_rowtop(hipStream_t s, const float* logits, int ldl, int ncols, int R, int W, const float* cum, float* cand_s,
                              float* cand_lp, int* cand_v) {
    if (R <= 0) return hipSuccess;
    if (ncols <= 0 || ncols > ldl || W < 1 || W > BEAM_MAX_W) return hipErrorInvalidValue;
    return launch_row_kernel<k_beam_rowtop<true>, k_beam_rowtop<false>>(s, R, ncols, 0, logits, ldl, ncols, W, cum, cand_s, cand_lp, cand_v);
}

hipError_t launch_beam_select(hipStream_t s, int G, int W, int ncols, const float* cand_s, const float* cand_lp, const int* cand_v,
                              float* cum, int* tok, int ldtok, int pos_out, int* par, int* htok, float* hlp) {
    if (G <= 0) return hipSuccess;
    if (W < 1 || W > BEAM_MAX_W || ncols <= 0 || pos_out >= ldtok) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_beam_select, dim3(G), dim3(SEL_THREADS), 0, s, W, ncols, cand_s, cand_lp, cand_v, cum, tok, ldtok, pos_out, par,
                       htok, hlp);
    return hipGetLastError();
}

namespace {
bool beam_con_ok(const ConstraintDev& c) {
    return c.S >= 1 && c.S <= CON_MAX_STATES && c.C >= 1 && c.C <= CON_MAX_CLASSES && c.KW >= 0 && c.KW <= CON_MAX_SLOTS / 32 && c.bias &&
           c.cls && c.slot && c.next && c.state && c.open && c.dead;
}
}  // namespace

hipError_t launch_beam_rowtop_constrained(hipStream_t s, const float* logits, int ldl, int ncols, int R, int W, const float* cum,
                                          const ConstraintDev& c, float* cand_s, float* cand_lp, int* cand_v, int* row_dead) {
    if (R <= 0) return hipSuccess;
    if (ncols <= 0 || ncols > ldl || W < 1 || W > BEAM_MAX_W || !beam_con_ok(c) || !row_dead) return hipErrorInvalidValue;
    // an unstaged row keeps Omega as a bitmap of its columns in LDS
    const size_t bitmap_bytes = sizeof(unsigned) * (size_t)((ncols + 31) / 32);
    if (bitmap_bytes > sizeof(float) * PICK_LDS_FLOATS) return hipErrorInvalidValue;
    return launch_row_kernel<k_beam_rowtop_constrained<true>, k_beam_rowtop_constrained<false>>(s, R, ncols, bitmap_bytes, logits, ldl, ncols, W,
                                                                                                cum, c, cand_s, cand_lp, cand_v, row_dead);
}

hipError_t launch_beam_select_constrained(hipStream_t s, int G, int W, int ncols, const float* cand_s, const float* cand_lp,
                                          const int* cand_v, const int* row_dead, const ConstraintDev& c, int* state_new, int* dead_new,
                                          float* cum, int* tok, int ldtok, int pos_out, int* par, int* htok, float* hlp) {
    if (G <= 0) return hipSuccess;
    if (W < 1 || W > BEAM_MAX_W || ncols <= 0 || pos_out >= ldtok || !beam_con_ok(c) || !row_dead || !state_new || !dead_new ||
        state_new == c.state || dead_new == c.dead)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_beam_select_constrained, dim3(G), dim3(SEL_THREADS), 0, s, W, ncols, cand_s, cand_lp, cand_v, row_dead, c, state_new,
                       dead_new, cum, tok, ldtok, pos_out, par, htok, hlp);
    return hipGetLastError();
}

hipError_t launch_beam_con_reorder(hipStream_t s, int R, int W, const ConstraintDev& c, const int* par, const int* htok, const int* row_dead,
                                   unsigned* open_dst) {
    if (R <= 0 || c.KW == 0) return hipSuccess;
    if (W < 1 || R % W || !beam_con_ok(c) || !open_dst || open_dst == c.open) return hipErrorInvalidValue;
    const long long n = (long long)R * c.KW;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_beam_con_reorder, dim3(blocks), dim3(256), 0, s, R, W, c.KW, par, htok, row_dead, c.slot, c.open, open_dst);
    return hipGetLastError();
}

hipError_t launch_beam_reorder(hipStream_t s, int L, int R, int W, int Hp, const int* par, const float* h_src, float* h_dst,
                               const float* c_src, float* c_dst) {
    if (R <= 0) return hipSuccess;
    if ((Hp & 3) || W < 1 || R % W) return hipErrorInvalidValue;
    const long long n = (long long)L * R * (Hp / 4);
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_beam_reorder, dim3(blocks), dim3(256), 0, s, L, R, W, Hp, par, h_src, h_dst, c_src, c_dst);
    return hipGetLastError();
}

hipError_t launch_beam_backtrace(hipStream_t s, int R, int W, int num, const int* par, const int* htok, const float* hlp, const float* cum,
                                 int* out_tok, float* out_lp, float* out_score) {
    if (R <= 0) return hipSuccess;
    if (W < 1 || R % W || num < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_beam_backtrace, dim3((R + 255) / 256), dim3(256), 0, s, R, W, num, par, htok, hlp, cum, out_tok, out_lp, out_score);
    return hipGetLastError();
}

hipError_t launch_feed_logprob(hipStream_t s, const float* logits, int ldl, int ncols, int R, const int* tok, int ldtok, int pos_tgt,
                               float* out_lp, int n, int i) {
    if (R <= 0) return hipSuccess;
    if (ncols <= 0 || ncols > ldl || i < 0 || i >= n || pos_tgt < 0 || pos_tgt >= ldtok) return hipErrorInvalidValue;
    return launch_row_kernel<k_feed_logprob<true>, k_feed_logprob<false>>(s, R, ncols, 0, logits, ldl, ncols, tok, ldtok, pos_tgt, out_lp, n, i);
}

hipError_t launch_dstate_rows(hipStream_t s, int L, int Rd, int Rs, int Hp, const int* rows, int div, const float* h_src, float* h_dst,
                              const float* c_src, float* c_dst, const int* tok_src, int ld_src, int off_src, int* tok_dst, int ld_dst,
                              int off_dst, int ntok) {
    if (Rd <= 0) return hipSuccess;
    if ((Hp & 3) || Rs <= 0 || div < 1 || ntok < 0 || off_src < 0 || off_dst < 0 || off_src + ntok > ld_src || off_dst + ntok > ld_dst ||
        (rows == nullptr && (long long)(Rd - 1) / div >= Rs))
        return hipErrorInvalidValue;
    const long long n = (long long)L * Rd * (Hp / 4) + (long long)Rd * ntok;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_dstate_rows, dim3(blocks), dim3(256), 0, s, L, Rd, Rs, Hp, rows, div, h_src, h_dst, c_src, c_dst, tok_src, ld_src,
                       off_src, tok_dst, ld_dst, off_dst, ntok);
    return hipGetLastError();
}

hipError_t launch_dstate_reset(hipStream_t s, long long n_state, float* hh, float* cc, long long n_tok, int* tok, int start) {
    if (n_state + n_tok <= 0) return hipSuccess;
    const int blocks = (int)std::min<long long>((n_state + n_tok + 255) / 256, 2048);
    hipLaunchKernelGGL(k_dstate_reset, dim3(blocks), dim3(256), 0, s, n_state, hh, cc, n_tok, tok, start);
    return hipGetLastError();
}

hipError_t launch_dstate_tokens(hipStream_t s, const int* tokens, int R, int n, int ncols, int start, int* tok, int ldtok, int off, int* err) {
    if (R <= 0 || n <= 0) return hipSuccess;
    if (tokens == nullptr || off < 0 || off + n > ldtok || start < 0 || start >= ncols) return hipErrorInvalidValue;
    const long long total = (long long)R * n;
    const int blocks = (int)std::min<long long>((total + 255) / 256, 1024);
    hipLaunchKernelGGL(k_dstate_tokens, dim3(blocks), dim3(256), 0, s, tokens, R, n, ncols, start, tok, ldtok, off, err);
    return hipGetLastError();
}

}  // namespace fsmg
