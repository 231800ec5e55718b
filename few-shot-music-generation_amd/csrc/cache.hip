// Support-set neural cache (include/fsmg.h fsmg_cache_*): the fused attention kernel and the kernel that files a pass's
// top-layer hidden states into a cache; k_cache_attend_self, the causal sibling over a row's own history.  The two
// attention kernels are one product loop (ca_key_tile), one online-softmax update (ca_update_masked) and one epilogue (ca_finish);
// they differ in the keys they walk and in the masks they build.
//
// k_cache_attend: p_cache(y) = sum_{i : v_i = y} exp(theta (d_i - d_max)) / sum_i exp(theta (d_i - d_max)), d_i = q . k_i over the
// Mg keys of the query's group, for up to 8 values of theta in one pass over the keys.  One 256-thread workgroup owns a tile of 32
// queries of ONE group (the host sorts the queries by group: CacheAttendArgs::slot_query / tile_group) and keeps them in LDS; its four
// waves walk the group's 16-key tiles round robin (wave w takes tiles w, w + 4, ...: a function of the group's entry count alone -- Mg, or n_g of a ragged cache).  Keys are the A operand
// and queries the B operand, so that lane l ends up with the scores of query l % 16 against keys l / 16 + {0, 4, 8, 12} of the tile: every
// lane runs an online softmax of ITS OWN (query, key subset) pair in registers -- one running maximum for all theta (theta >= 0), a
// denominator and a numerator per theta -- and nothing crosses lanes inside the key loop.  The score matrix never leaves the
// registers.  The partial (max, sums) are merged in a fixed order: lanes 16 / 32 apart by shuffles, then the four waves through LDS by
// one thread per query.  A key index >= the entry count is skipped (masked, not scored as zero).  No atomics.  A query's bits depend on its vector,
// its group's entries and theta alone: each score is an accumulator element of its own, and the merge tree does not depend on the slot
// a query got.
//
// Precision.  theta d reaches tens of units, and an error of e in theta (d_i - d_max) is a relative error of e in that entry's mass.
// With scores accumulated in fp32 over 512 units p_cache was measured 5.6e-6 off fp64 at theta (d_max - d_min) = 40, and even a
// correctly rounded fp32 score of magnitude 8 is up to 5e-7 off.  So the products run on v_mfma_f64_16x16x4_f64 -- the fp32 inputs
// widened exactly, every product exact, fp64 accumulation: half the fp32 pipe's rate, and the one way to scores that are not the
// error budget -- and the exponent stays in fp64 up to the last step:
//   u = theta log2(e);  S = ceil(u m), m the running maximum (an integer shift: changing it rescales the sums by an exact power of two);
//   t = u d - S in fp64 (<= 0),  hi = fl32(t),  lo = fl32(t - hi);   mass = exp2f(hi) (1 + lo ln 2), summed in fp64.
// What is left is exp2f's own rounding, ~1e-7 per entry.
#include "fsmg_kernels.h"

namespace fsmg {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int CA_QT = CACHE_ATTEND_QT;      // queries per workgroup: two 16-column B operands, so a key load feeds two MFMAs
constexpr int CA_WAVES = 4;
constexpr int CA_PAD = 4;                   // floats behind a query row in LDS: rows 16 B apart in the banks

// a partial softmax over some of a group's keys: the sums are sum_i 2^(u_k d_i - ceil(u_k m)), m the largest d among them
struct CaState {
    double m = -INFINITY;
    double den[CACHE_MAX_THETA] = {}, num[CACHE_MAX_THETA] = {};
};

// 2^(ceil(u m_from) - ceil(u m_to)), m_to >= m_from: exact; an empty partial (m_from = -inf, sums 0) scales by 0, u = 0 included
__device__ __forceinline__ double ca_scale(double u, double m_from, double m_to) {
    if (m_from == -INFINITY) return 0.0;
    return ldexp(1.0, (int)fmax(ceil(u * m_from) - ceil(u * m_to), -4000.0));
}

// the four scores of a lane (values v) into its running state; bit i of `mask` says that score i counts for this lane's query (a
// tail key, a key the position does not see: skipped, not scored as zero)
__device__ __forceinline__ void ca_update_masked(CaState& st, const f64x4& d, unsigned mask, const int v[4], int y, const double* u,
                                                 int n_theta) {
    double mt = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (mask >> i & 1u) mt = fmax(mt, d[i]);
    if (mt > st.m) {
#pragma unroll
        for (int k = 0; k < CACHE_MAX_THETA; ++k)
            if (k < n_theta) {
                const double sc = ca_scale(u[k], st.m, mt);
                st.den[k] *= sc; st.num[k] *= sc;
            }
        st.m = mt;
    }
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k) {
        if (k >= n_theta) continue;
        const double S = ceil(u[k] * st.m);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!(mask >> i & 1u)) continue;            // a masked key has no mass
            const double e = ca_exp2(fma(u[k], d[i], -S));
            st.den[k] += e;
            if (v[i] == y) st.num[k] += e;
        }
    }
}

// (st) <- (st) merged with the partial (mo, deno, numo), in this order
__device__ __forceinline__ void ca_merge(CaState& st, double mo, const double* deno, const double* numo, const double* u, int n_theta) {
    const double m = fmax(st.m, mo);
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k)
        if (k < n_theta) {
            const double sa = ca_scale(u[k], st.m, m), sb = ca_scale(u[k], mo, m);
            st.den[k] = st.den[k] * sa + deno[k] * sb;
            st.num[k] = st.num[k] * sa + numo[k] * sb;
        }
    st.m = m;
}

__device__ __forceinline__ double ca_shfl(double x, int off) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __shfl_xor(lo, off, 64); hi = __shfl_xor(hi, off, 64);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void ca_merge_lanes(CaState& st, int off, const double* u, int n_theta) {
    const double mo = ca_shfl(st.m, off);
    double deno[CACHE_MAX_THETA], numo[CACHE_MAX_THETA];
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k) {
        deno[k] = ca_shfl(st.den[k], off);
        numo[k] = ca_shfl(st.num[k], off);
    }
    ca_merge(st, mo, deno, numo, u, n_theta);
}

// 16 keys x 32 (TWO) or 16 queries x 16 k: the key fragment feeds both query halves; k order x, y, z, w
template <bool TWO>
__device__ __forceinline__ void ca_mfma4(f64x4& acc0, f64x4& acc1, const float4& kv, const float4& b0, const float4& b1) {
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.x, (double)b0.x, acc0, 0, 0, 0);
    if (TWO) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.x, (double)b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.y, (double)b0.y, acc0, 0, 0, 0);
    if (TWO) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.y, (double)b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.z, (double)b0.z, acc0, 0, 0, 0);
    if (TWO) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.z, (double)b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.w, (double)b0.w, acc0, 0, 0, 0);
    if (TWO) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64((double)kv.w, (double)b1.w, acc1, 0, 0, 0);
}

// four floats at p, units c .. c + 3 of a vector of H: a pad unit reads as an exact zero whatever the memory holds
__device__ __forceinline__ float4 ca_load4_h(const float* p, int c, int H) {
    float4 v = *reinterpret_cast<const float4*>(p);
    if (c + 0 >= H) v.x = 0.0f;
    if (c + 1 >= H) v.y = 0.0f;
    if (c + 2 >= H) v.z = 0.0f;
    if (c + 3 >= H) v.w = 0.0f;
    return v;
}

// one 16-key tile against the 32 queries in LDS, groups of 16 in increasing k; PADS: the key's pad units are masked (a vector of the
// pass).  Two k groups per trip by hand: the loads of the second go out before the first one's products; a requested unroll of this
// loop is refused by the compiler.
template <bool PADS>
__device__ __forceinline__ void ca_key_tile(const float* __restrict__ kp, const float* qp0, const float* qp1, int Hp, int H, int c0,
                                            f64x4& acc0, f64x4& acc1) {
    int k = 0;
    for (; k + 32 <= Hp; k += 32) {
        const float4 kv = PADS ? ca_load4_h(kp + k, c0 + k, H) : *reinterpret_cast<const float4*>(kp + k);
        const float4 kw = PADS ? ca_load4_h(kp + k + 16, c0 + k + 16, H) : *reinterpret_cast<const float4*>(kp + k + 16);
        const float4 b0 = *reinterpret_cast<const float4*>(qp0 + k), c0v = *reinterpret_cast<const float4*>(qp0 + k + 16);
        const float4 b1 = *reinterpret_cast<const float4*>(qp1 + k), c1v = *reinterpret_cast<const float4*>(qp1 + k + 16);
        ca_mfma4<true>(acc0, acc1, kv, b0, b1);
        ca_mfma4<true>(acc0, acc1, kw, c0v, c1v);
    }
    if (k < Hp) {
        const float4 kv = PADS ? ca_load4_h(kp + k, c0 + k, H) : *reinterpret_cast<const float4*>(kp + k);
        const float4 b0 = *reinterpret_cast<const float4*>(qp0 + k);
        const float4 b1 = *reinterpret_cast<const float4*>(qp1 + k);
        ca_mfma4<true>(acc0, acc1, kv, b0, b1);
    }
}

// what the four waves of a workgroup hand to the threads that merge them
struct CaMerge {
    double m[CA_WAVES][CA_QT];
    double den[CA_WAVES][CACHE_MAX_THETA][CA_QT], num[CA_WAVES][CACHE_MAX_THETA][CA_QT];
};

// The end of an attention workgroup (all 256 threads call it): the four key subsets of a wave as (0 + 1) + (2 + 3), read from the
// lanes with l / 16 == 0; then the four waves through `mg` -- the bytes of the query tile, behind a barrier -- merged in the order
// 0, 1, 2, 3 by thread s < CA_QT for slot s.  owner(s) is that slot's index into a row of `out` ([n_theta][n]), negative for an
// empty slot: out[k * n + owner(s)] = num_k / den_k, exactly 0 where no mass met the target.
template <class Owner>
__device__ __forceinline__ void ca_finish(CaState& st0, CaState& st1, CaMerge& mg, const double* u, int n_theta, float* out, long long n,
                                          Owner&& owner) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane & 15, ks = lane >> 4;
    ca_merge_lanes(st0, 16, u, n_theta); ca_merge_lanes(st0, 32, u, n_theta);
    ca_merge_lanes(st1, 16, u, n_theta); ca_merge_lanes(st1, 32, u, n_theta);
    __syncthreads();                                 // every wave is done with the query tile
    if (ks == 0) {
        mg.m[wave][kq] = st0.m; mg.m[wave][16 + kq] = st1.m;
#pragma unroll
        for (int k = 0; k < CACHE_MAX_THETA; ++k) {
            mg.den[wave][k][kq] = st0.den[k]; mg.den[wave][k][16 + kq] = st1.den[k];
            mg.num[wave][k][kq] = st0.num[k]; mg.num[wave][k][16 + kq] = st1.num[k];
        }
    }
    __syncthreads();
    if (tid >= CA_QT) return;
    const long long q = owner(tid);
    if (q < 0) return;
    CaState st;
    for (int w = 0; w < CA_WAVES; ++w) {
        double deno[CACHE_MAX_THETA], numo[CACHE_MAX_THETA];
#pragma unroll
        for (int k = 0; k < CACHE_MAX_THETA; ++k) { deno[k] = mg.den[w][k][tid]; numo[k] = mg.num[w][k][tid]; }
        ca_merge(st, mg.m[w][tid], deno, numo, u, n_theta);
    }
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k)
        if (k < n_theta) out[k * n + q] = st.num[k] == 0.0 ? 0.0f : (float)(st.num[k] / st.den[k]);
}

// where query id q lives and what its target is (CacheAttendArgs)
__device__ __forceinline__ long long ca_query_row(const CacheAttendArgs& a, int q) {
    return a.B > 0 ? (long long)(q % a.T + 1) * a.B + q / a.T : (long long)q;
}
__device__ __forceinline__ int ca_target(const CacheAttendArgs& a, int q) {
    return a.B > 0 ? a.tgt[(long long)(q % a.T) * a.B + q / a.T] : a.tgt[q];
}

__global__ __launch_bounds__(256) void k_cache_attend(CacheAttendArgs a) {
    // the query tile [CA_QT][Hp + CA_PAD] floats; once the key loop is over the same bytes hold the waves' partials (CaMerge): at
    // hidden 512 a workgroup then needs 66 KiB, and two of them share a CU's 160 KiB
    extern __shared__ double ca_lds[];
    float* ca_q = reinterpret_cast<float*>(ca_lds);
    CaMerge& mg = *reinterpret_cast<CaMerge*>(ca_lds);
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hp = a.Hp, Mg = a.Mg, ldl = Hp + CA_PAD, n_theta = a.n_theta;
    const int g = a.tile_group[tile];
    const int* slots = a.slot_query + (long long)tile * CA_QT;
    double theta[CACHE_MAX_THETA];                  // u = theta log2(e)
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k) theta[k] = (double)a.theta[k] * CA_LOG2E;

    // the tile's queries into LDS, an empty slot as zeros
    const int c4n = Hp >> 2;
    for (int idx = tid; idx < CA_QT * c4n; idx += 256) {
        const int s = idx / c4n, c4 = idx - s * c4n;
        const int q = slots[s];
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q >= 0) v = *reinterpret_cast<const float4*>(a.Q + ca_query_row(a, q) * a.ldq + 4 * c4);
        *reinterpret_cast<float4*>(ca_q + s * ldl + 4 * c4) = v;
    }
    __syncthreads();

    const int kq = lane & 15, ks = lane >> 4;
    const float* kg = a.keys + (long long)g * Mg * Hp;
    const int* vg = a.vals + (long long)g * Mg;
    const int q0 = slots[kq], q1 = slots[16 + kq];
    const int y0 = q0 >= 0 ? ca_target(a, q0) : -1, y1 = q1 >= 0 ? ca_target(a, q1) : -1;       // (values are >= 0: -1 never hits)
    CaState st0, st1;
    const float* qp0 = ca_q + kq * ldl + 4 * ks;
    const float* qp1 = qp0 + 16 * ldl;
    // the group's entries: Mg stays the stride, ng is the extent (g is the tile's one group: a uniform load, uniform trip counts)
    const int ng = a.count ? a.count[g] : Mg;
    const int n_kt = (ng + 15) >> 4;
    for (int kt = wave; kt < n_kt; kt += CA_WAVES) {
        // lane l loads key row l % 16 of the tile (a tail row: the group's last key, in bounds, masked below), k = 16 j + 4 (l / 16) .. + 3
        const int krow = min(kt * 16 + kq, ng - 1);
        const float* kp = kg + (long long)krow * Hp + 4 * ks;
        f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        ca_key_tile<false>(kp, qp0, qp1, Hp, Hp, 4 * ks, acc0, acc1);
        // accumulator register i of lane l (the fp64 instruction's layout): key 4 i + l / 16 of the tile against query l % 16
        const int kbase = kt * 16 + ks;
        int v[4];
        unsigned m = 0;                             // a tail key has no mass
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = vg[min(kbase + 4 * i, ng - 1)];
            if (kbase + 4 * i < ng) m |= 1u << i;
        }
        ca_update_masked(st0, acc0, m, v, y0, theta, n_theta);
        ca_update_masked(st1, acc1, m, v, y1, theta, n_theta);
    }
    ca_finish(st0, st1, mg, theta, n_theta, a.out, a.n, [&](int s) { return (long long)slots[s]; });
}

// ---------------------------------------------------------------- self-cache (fsmg_kernels.h CacheSelfArgs)
__global__ __launch_bounds__(256) void k_cache_attend_self(CacheSelfArgs a) {
    // k_cache_attend's LDS plan: the query tile, then the waves' partials over the same bytes
    extern __shared__ double ca_lds[];
    float* ca_q = reinterpret_cast<float*>(ca_lds);
    CaMerge& mg = *reinterpret_cast<CaMerge*>(ca_lds);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Hp = a.Hp, H = a.H, Mg = a.Mg, T = a.T, W = a.W, ldl = Hp + CA_PAD, n_theta = a.n_theta;
    const int tiles_per_row = (T + CA_QT - 1) / CA_QT;
    const int r = blockIdx.x / tiles_per_row, t0 = (blockIdx.x - r * tiles_per_row) * CA_QT;
    const float* vr = a.V + (long long)r * a.vs_r;
    const int* yr = a.val + (long long)r * a.ys_r;
    double theta[CACHE_MAX_THETA];                  // u = theta log2(e)
#pragma unroll
    for (int k = 0; k < CACHE_MAX_THETA; ++k) theta[k] = (double)a.theta[k] * CA_LOG2E;

    // positions t0 .. t0 + 31 of the row into LDS with their pad units zeroed; a position past the row's end as zeros
    const int c4n = Hp >> 2;
    for (int idx = tid; idx < CA_QT * c4n; idx += 256) {
        const int s = idx / c4n, c4 = idx - s * c4n;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t0 + s < T) v = ca_load4_h(vr + (long long)(t0 + s) * a.vs_t + 4 * c4, 4 * c4, H);
        *reinterpret_cast<float4*>(ca_q + s * ldl + 4 * c4) = v;
    }
    __syncthreads();

    const int kq = lane & 15, ks = lane >> 4;
    const int ta = t0 + kq, tb = t0 + 16 + kq;      // this lane's two positions
    const int y0 = ta < T ? yr[(long long)ta * a.ys_t] : -1, y1 = tb < T ? yr[(long long)tb * a.ys_t] : -1;
    CaState st0, st1;
    const float* qp0 = ca_q + kq * ldl + 4 * ks;
    const float* qp1 = qp0 + 16 * ldl;
    // phase one: the group's support keys, every one visible to every position of the row (k_cache_attend's walk)
    // (r is the workgroup's one row, so its group and the group's entry count ng are uniform; Mg stays the stride)
    const int g = Mg > 0 && a.row_group ? a.row_group[r] : 0;
    const int ng = Mg > 0 && a.count ? a.count[g] : Mg;
    const int n_kt = (ng + 15) >> 4;
    if (Mg > 0) {
        const float* kg = a.keys + (long long)g * Mg * Hp;
        const int* vg = a.vals + (long long)g * Mg;
        for (int kt = wave; kt < n_kt; kt += CA_WAVES) {
            const int krow = min(kt * 16 + kq, ng - 1);
            f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
            ca_key_tile<false>(kg + (long long)krow * Hp + 4 * ks, qp0, qp1, Hp, H, 4 * ks, acc0, acc1);
            const int kbase = kt * 16 + ks;
            int v[4];
            unsigned m = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = vg[min(kbase + 4 * i, ng - 1)];
                if (kbase + 4 * i < ng) m |= 1u << i;
            }
            ca_update_masked(st0, acc0, ta < T ? m : 0u, v, y0, theta, n_theta);
            ca_update_masked(st1, acc1, tb < T ? m : 0u, v, y1, theta, n_theta);
        }
    }
    // phase two: the row's own keys lo .. hi - 1, the only ones some position of this tile sees (key i is seen by position t when
    // t - W <= i < t); own tile j goes to wave (n_kt + j) % 4, so the round robin goes on where the support keys left it
    const int lo = max(0, t0 - W), hi = min(t0 + CA_QT - 1, T - 1);
    const int n_ot = hi > lo ? (hi - lo + 15) >> 4 : 0;
    for (int j = (wave + CA_WAVES - (n_kt & 3)) & 3; j < n_ot; j += CA_WAVES) {
        // lane l loads own key row l % 16 of the tile (a tail row: key hi - 1, in bounds, masked below)
        const int krow = min(lo + j * 16 + kq, hi - 1);
        f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        ca_key_tile<true>(vr + (long long)krow * a.vs_t + 4 * ks, qp0, qp1, Hp, H, 4 * ks, acc0, acc1);
        const int kbase = lo + j * 16 + ks;
        int v[4];
        unsigned m0 = 0, m1 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ki = kbase + 4 * i;           // (ki >= hi is >= every position of the tile: never visible)
            v[i] = yr[(long long)min(ki, hi - 1) * a.ys_t];
            if (ta < T && ki < ta && ki >= ta - W) m0 |= 1u << i;
            if (tb < T && ki < tb && ki >= tb - W) m1 |= 1u << i;
        }
        ca_update_masked(st0, acc0, m0, v, y0, theta, n_theta);
        ca_update_masked(st1, acc1, m1, v, y1, theta, n_theta);
    }
    ca_finish(st0, st1, mg, theta, n_theta, a.out, (long long)a.n_rows * T,
              [&](int s) { return t0 + s < T ? (long long)r * T + t0 + s : -1LL; });
}

// Hs1: slot 1 of the pass's top-layer hidden states, time-major [T][B][Hp]; Y [T][B].  Pass row b is row r0 + b of the cache's
// [rows][T] entries (group-major: group = row / rows_per_group, entry = (row % rows_per_group) * T + t).  Pad units are written as zeros.
__global__ __launch_bounds__(256) void k_cache_fill(const float* __restrict__ Hs1, const int* __restrict__ Y, int B, int T, int H, int Hp,
                                                    long long r0, float* __restrict__ keys, int* __restrict__ vals) {
    const int c4n = Hp >> 2;
    const long long total = (long long)T * B * c4n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / c4n;                // t * B + b
        const int c4 = (int)(idx - row * c4n);
        const int t = (int)(row / B), b = (int)(row - (long long)t * B);
        const int c = 4 * c4;
        const float4 v = ca_load4_h(Hs1 + row * Hp + c, c, H);
        const long long e = (r0 + b) * T + t;
        *reinterpret_cast<float4*>(keys + e * Hp + c) = v;
        if (c4 == 0) vals[e] = Y[row];
    }
}

// k_cache_fill for a ragged cache (fsmg_kernels.h launch_cache_fill_len): position t of pass row b becomes entry dst[b] + t of the flat
// [G * Mg] entries when t < len[b], and is dropped otherwise.  The host makes dst, so that a group's rows follow each other without
// gaps: len[b] <= T and the group's capacity Mg = rows_per_group * T keep every index inside the group.
__global__ __launch_bounds__(256) void k_cache_fill_len(const float* __restrict__ Hs1, const int* __restrict__ Y, int B, int T, int H, int Hp,
                                                        const int* __restrict__ len, const int* __restrict__ dst, float* __restrict__ keys,
                                                        int* __restrict__ vals) {
    const int c4n = Hp >> 2;
    const long long total = (long long)T * B * c4n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long row = idx / c4n;                // t * B + b
        const int c4 = (int)(idx - row * c4n);
        const int t = (int)(row / B), b = (int)(row - (long long)t * B);
        if (t >= len[b]) continue;                      // behind the song's end: no entry
        const int c = 4 * c4;
        const float4 v = ca_load4_h(Hs1 + row * Hp + c, c, H);
        const long long e = (long long)dst[b] + t;
        *reinterpret_cast<float4*>(keys + e * Hp + c) = v;
        if (c4 == 0) vals[e] = Y[row];
    }
}

// ---------------------------------------------------------------- cache-conditioned generation, stage one (fsmg_kernels.h)
// One wave: 16 keys of a chunk against the 16 (or 32) queries of a tile, operands straight from global memory -- a wave's key
// fragment is read once, and the tile's queries are a few KiB that every wave of the group reads and the caches keep.  Four k groups
// per trip so that eight (twelve) 16-byte loads are in flight: at a decode step one wave per SIMD is all the occupancy there is.
// The k order is k_cache_attend's: groups of 16 in increasing k, x, y, z, w inside a group.
template <bool TWO>
__device__ __forceinline__ void cs_tile(const float* __restrict__ kp, const float* __restrict__ qp0, const float* __restrict__ qp1, int Hp,
                                        f64x4& acc0, f64x4& acc1) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int k = 0;
    for (; k + 64 <= Hp; k += 64) {
        float4 kv[4], b0[4], b1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            kv[j] = *reinterpret_cast<const float4*>(kp + k + 16 * j);
            b0[j] = *reinterpret_cast<const float4*>(qp0 + k + 16 * j);
            b1[j] = TWO ? *reinterpret_cast<const float4*>(qp1 + k + 16 * j) : zero;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ca_mfma4<TWO>(acc0, acc1, kv[j], b0[j], b1[j]);
    }
    for (; k < Hp; k += 16) {
        const float4 kv = *reinterpret_cast<const float4*>(kp + k);
        const float4 b0 = *reinterpret_cast<const float4*>(qp0 + k);
        const float4 b1 = TWO ? *reinterpret_cast<const float4*>(qp1 + k) : zero;
        ca_mfma4<TWO>(acc0, acc1, kv, b0, b1);
    }
}

__global__ __launch_bounds__(64) void k_cache_scores(CacheScoresArgs a, int n_chunks) {
    const int tile = blockIdx.x / n_chunks, chunk = blockIdx.x - tile * n_chunks;
    const int lane = threadIdx.x, kq = lane & 15, ks = lane >> 4;
    const int Hp = a.Hp, Mg = a.Mg;
    const int g = a.tile_group[tile];
    const int ng = a.count ? a.count[g] : Mg;       // the tile's one group: Mg stays the stride of keys and of D
    if (chunk * CACHE_GEN_CHUNK >= ng) return;      // a chunk wholly behind the count (wave-uniform: one wave per block)
    const int* slots = a.slot_query + (long long)tile * CACHE_ATTEND_QT;
    const int q0 = slots[kq], q1 = slots[16 + kq];
    const bool two = slots[16] >= 0;                // the slots fill in order: a wave-uniform choice
    const int qa = slots[0];                        // (never empty) an empty slot reads this row, in bounds, and stores nothing
    // lane l loads key row l % 16 of the chunk (a tail row: the group's last key, in bounds, not stored), k = 16 j + 4 (l / 16) .. + 3
    const int krow = min(chunk * CACHE_GEN_CHUNK + kq, ng - 1);
    const float* kp = a.keys + ((long long)g * Mg + krow) * Hp + 4 * ks;
    const float* qp0 = a.Q + (long long)(q0 >= 0 ? q0 : qa) * a.ldq + 4 * ks;
    const float* qp1 = a.Q + (long long)(q1 >= 0 ? q1 : qa) * a.ldq + 4 * ks;
    f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    if (two) cs_tile<true>(kp, qp0, qp1, Hp, acc0, acc1);
    else cs_tile<false>(kp, qp0, qp1, Hp, acc0, acc1);
    // accumulator register i of lane l: key 4 i + l / 16 of the chunk against query l % 16
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = chunk * CACHE_GEN_CHUNK + 4 * i + ks;
        if (key >= ng) continue;                    // a tail key has no score
        if (q0 >= 0) a.D[(long long)q0 * Mg + key] = acc0[i];
        if (two && q1 >= 0) a.D[(long long)q1 * Mg + key] = acc1[i];
    }
}

// ---------------------------------------------------------------- decode-time self-cache (fsmg_kernels.h)
__global__ __launch_bounds__(256) void k_self_file(const float* __restrict__ h_out, int R, int H, int Hp, float* __restrict__ own_keys,
                                                   int NP, int p) {
    const int c4n = Hp >> 2;
    const long long total = (long long)R * c4n;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int r = (int)(idx / c4n), c4 = (int)(idx - (long long)r * c4n);
        *reinterpret_cast<float4*>(own_keys + ((long long)r * NP + p) * Hp + 4 * c4) = ca_load4_h(h_out + (long long)r * Hp + 4 * c4, 4 * c4, H);
    }
}

__global__ __launch_bounds__(64) void k_self_scores(SelfScoresArgs a, int n_chunks) {
    const int r = blockIdx.x / n_chunks, chunk = blockIdx.x - r * n_chunks;
    const int len = a.row_len ? a.row_len[r] : a.len;
    const int n = min(len, a.W), lo = len - n;
    if (chunk * 16 >= n) return;                    // (wave-uniform)
    const int lane = threadIdx.x, kq = lane & 15, ks = lane >> 4;
    const int j = chunk * 16 + kq;
    // a tail lane reads the row's last visible key, in bounds, and stores nothing
    const float* kp = a.own_keys + ((long long)r * a.NP + lo + min(j, n - 1)) * a.Hp + 4 * ks;
    const float* qp = a.Q + (long long)r * a.ldq + 4 * ks;
    double acc = 0.0;
    for (int k = 0; k < a.Hp; k += 16) {
        const float4 kv = *reinterpret_cast<const float4*>(kp + k);
        const float4 qv = *reinterpret_cast<const float4*>(qp + k);
        acc = fma((double)kv.x, (double)qv.x, acc);
        acc = fma((double)kv.y, (double)qv.y, acc);
        acc = fma((double)kv.z, (double)qv.z, acc);
        acc = fma((double)kv.w, (double)qv.w, acc);
    }
    acc += ca_shfl(acc, 16);                        // (0 + 1), (2 + 3)
    acc += ca_shfl(acc, 32);                        // ((0 + 1) + (2 + 3)): the same bits in every lane of a key
    if (ks == 0 && j < n) a.D2[(long long)r * a.ldo + j] = acc;
}

}  // namespace

hipError_t launch_self_file(hipStream_t s, const float* h_out, int R, int H, int Hp, float* own_keys, int NP, int p) {
    if (R <= 0) return hipSuccess;
    if ((Hp & 3) != 0 || H < 1 || H > Hp || p < 0 || p >= NP) return hipErrorInvalidValue;
    const long long total = (long long)R * (Hp >> 2);
    hipLaunchKernelGGL(k_self_file, dim3((unsigned)std::min<long long>((total + 255) / 256, 4096)), dim3(256), 0, s, h_out, R, H, Hp, own_keys, NP, p);
    return hipGetLastError();
}

hipError_t launch_self_scores(hipStream_t s, const SelfScoresArgs& a) {
    if (a.R <= 0) return hipSuccess;
    const int cap = std::min(a.W, a.NP);
    if (a.W < 1 || a.NP < 1 || a.Hp < 16 || (a.Hp & 15) != 0 || (a.ldq & 3) != 0 || a.ldo < cap || (!a.row_len && (a.len < 0 || a.len > a.NP)))
        return hipErrorInvalidValue;
    const int most = a.row_len ? cap : std::min(a.len, cap);       // the longest visible set of the call
    const long long n_chunks = (most + 15) / 16;
    if (n_chunks == 0) return hipSuccess;
    if (n_chunks * a.R > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_self_scores, dim3((unsigned)(n_chunks * a.R)), dim3(64), 0, s, a, (int)n_chunks);
    return hipGetLastError();
}

size_t cache_attend_lds_bytes(int Hp) { return std::max(sizeof(float) * (size_t)CA_QT * (Hp + CA_PAD), sizeof(CaMerge)); }

hipError_t launch_cache_attend(hipStream_t s, const CacheAttendArgs& a) {
    if (a.n_tiles <= 0) return hipSuccess;
    if (a.Mg < 1 || a.Hp < 16 || (a.Hp & 15) != 0 || a.n_theta < 1 || a.n_theta > CACHE_MAX_THETA || (a.ldq & 3) != 0 || a.n < 1)
        return hipErrorInvalidValue;
    const size_t lds = cache_attend_lds_bytes(a.Hp);
    if (lds > 64 * 1024) {                  // hidden sizes above 508: more dynamic LDS than a launch gets by default (160 KiB per CU)
        const hipError_t e = hipFuncSetAttribute((const void*)k_cache_attend, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_cache_attend, dim3(a.n_tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cache_attend_self(hipStream_t s, const CacheSelfArgs& a) {
    if (a.n_rows <= 0 || a.T <= 0) return hipSuccess;
    const long long tiles = (long long)a.n_rows * ((a.T + CA_QT - 1) / CA_QT);
    if (a.Mg < 0 || a.Hp < 16 || (a.Hp & 15) != 0 || a.H < 1 || a.H > a.Hp || a.n_theta < 1 || a.n_theta > CACHE_MAX_THETA || a.W < 1 ||
        (a.vs_r & 3) != 0 || (a.vs_t & 3) != 0 || tiles > 0x7FFFFFFFLL)
        return hipErrorInvalidValue;
    const size_t lds = cache_attend_lds_bytes(a.Hp);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_cache_attend_self, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_cache_attend_self, dim3((unsigned)tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_cache_scores(hipStream_t s, const CacheScoresArgs& a) {
    if (a.n_tiles <= 0) return hipSuccess;
    const long long n_chunks = ((long long)a.Mg + CACHE_GEN_CHUNK - 1) / CACHE_GEN_CHUNK;
    if (a.Mg < 1 || a.Hp < 16 || (a.Hp & 15) != 0 || (a.ldq & 3) != 0 || n_chunks * a.n_tiles > 0x7FFFFFFFLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cache_scores, dim3((unsigned)(n_chunks * a.n_tiles)), dim3(64), 0, s, a, (int)n_chunks);
    return hipGetLastError();
}

hipError_t launch_cache_fill(hipStream_t s, const float* Hs1, const int* Y, int B, int T, int H, int Hp, long long r0, float* keys,
                             int* vals) {
    if (B <= 0 || T <= 0) return hipSuccess;
    if ((Hp & 3) != 0) return hipErrorInvalidValue;
    const long long total = (long long)T * B * (Hp >> 2);
    const int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_cache_fill, dim3(blocks), dim3(256), 0, s, Hs1, Y, B, T, H, Hp, r0, keys, vals);
    return hipGetLastError();
}

hipError_t launch_cache_fill_len(hipStream_t s, const float* Hs1, const int* Y, int B, int T, int H, int Hp, const int* len, const int* dst,
                                 float* keys, int* vals) {
    if (B <= 0 || T <= 0) return hipSuccess;
    if ((Hp & 3) != 0 || !len || !dst) return hipErrorInvalidValue;
    const long long total = (long long)T * B * (Hp >> 2);
    const int blocks = (int)std::min<long long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_cache_fill_len, dim3(blocks), dim3(256), 0, s, Hs1, Y, B, T, H, Hp, len, dst, keys, vals);
    return hipGetLastError();
}

}  // namespace fsmg
