// fp32 GEMMs for gfx950: k_gemm_bx3 (default) assembles every fp32 product from bf16 pieces on v_mfma_f32_32x32x16_bf16
// (16x the fp32 MFMA's rate; exact three-way operand split, six products, fp32 accumulation -- see the block comment above
// it), k_gemm / k_gemm_staged / k_gemm_queue run on v_mfma_f32_32x32x2_f32 (exact fp32, 157 TF peak).  The notes below
// describe the fp32-MFMA kernels; tiling, epilogue, split-K and tile order are shared.
//
// One kernel template serves every dense contraction of the LSTM-baseline step
// (DESIGN.md "Kernels"): the hoisted input projection with the embedding gather fused
// into the A-operand load, the vocabulary projection, and their backward pairs (dlogits is
// materialised once by the cross-entropy kernel: an earlier version recomputed
// exp(logit - lse) - onehot inside the operand loads of two GEMMs, 4x per element, and was
// slower).
//
// Tiling: 128x128 block tile, BK = 16, 256 threads = 4 wave64 as 2x2, each wave owns a
// 64x64 sub-tile = 2x2 MFMA 32x32 tiles (64 accumulator VGPRs).  Two kernels:
//   * k_gemm (the default, "main kernel" below): dense lane-linear LDS tiles, k-contiguous sources stored
//     untransposed and read with ds_read_b128 under a permuted contraction order, branch-free steady loop;
//   * k_gemm_staged (first version; kept for the x-contiguous operand whose K rows are GATHERED, dKx): both
//     operands K-major in LDS ([k][x], row stride 132 floats for 16-byte copies / 129 for k-contiguous sources
//     that are transposed on the way in with 4 ds_write_b32), predicated loads.
// Both: global loads for tile t+1 are issued before the MFMAs of tile t (register prefetch) and written to the
// other LDS buffer afterwards, one barrier per K tile; blocks are numbered so that the 8 XCDs (block b -> XCD
// b % 8 as observed on MI355X) each walk a contiguous range of tiles and share operand panels in their private L2.
#include "fsmg_kernels.h"
#include "gemm_edge.h"
#include <cstdlib>
#include <algorithm>
#include <type_traits>

namespace fsmg {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

#ifndef FSMG_GEMM_BK
#define FSMG_GEMM_BK 16
#endif
// BK = 16: 34 KiB LDS and <=104 VGPRs per block -> 4 resident blocks (16 waves) per CU, which covers the
// per-tile barrier and the prologue/epilogue bubbles better than 2 blocks of BK = 32 (measured +5..15 % per GEMM)
#ifndef FSMG_GEMM_BM
#define FSMG_GEMM_BM 128
#endif
constexpr int BM = FSMG_GEMM_BM, BN = 128, BK = FSMG_GEMM_BK;   // BM in {128, 256}, BK in {16, 32}
constexpr int NTHREADS = 2 * BM;                       // one wave64 per 64x64 sub-tile: (BM/64) x 2 waves
constexpr int NWAVES = NTHREADS / 64;
constexpr int KQ = BK / 4;                             // float4 slots along k in a KC tile row
// 16-byte loads per thread for an operand tile of XW rows/columns
template <int XW> struct Nld { static constexpr int v = XW * BK / 4 / NTHREADS; };
// LDS row strides: KC tiles are scattered with ds_write_b32 (stride = 1 mod 32 -> conflict free), XC tiles are
// copied with ds_write_b128 (stride a multiple of 4 floats)
template <int MODE, int XW> struct TileLd { static constexpr int v = (MODE == OP_KC) ? XW + 1 : XW + 4; };

// ---- KC source: tile [128 x][32 k], k contiguous.  thread -> rows x = tid/8 + 32*i, k quad kq = tid%8
template <int XW>
struct KcLoader {
    static constexpr int NLD = Nld<XW>::v, LD = XW + 1;
    const float* rowp[NLD];
    int kq;
    __device__ __forceinline__ void init(const float* src, int ld, int X, int x0, const int* gather, int tid) {
        kq = tid % KQ;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int x = x0 + (tid / KQ) + (NTHREADS / KQ) * i;
            bool ok = x < X;
            long long row = ok ? (gather ? (long long)gather[x] : (long long)x) : 0;
            rowp[i] = ok ? src + row * ld : nullptr;
        }
    }
    __device__ __forceinline__ void load(float4 (&r)[NLD], int k0, int kend) const {
        int k = k0 + 4 * kq;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rowp[i] != nullptr && k < kend) v = *reinterpret_cast<const float4*>(rowp[i] + k);
            r[i] = v;
        }
    }
    __device__ __forceinline__ void store(float* lds, const float4 (&r)[NLD], int tid) const {
        float* base = lds + (4 * kq) * LD + (tid / KQ);
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            base[0 * LD + (NTHREADS / KQ) * i] = r[i].x;
            base[1 * LD + (NTHREADS / KQ) * i] = r[i].y;
            base[2 * LD + (NTHREADS / KQ) * i] = r[i].z;
            base[3 * LD + (NTHREADS / KQ) * i] = r[i].w;
        }
    }
};

// ---- XC source: tile [32 k][128 x], x contiguous.  thread -> k rows tid/32 + 8*i, x quad xq = tid%32
template <int XW>
struct XcLoader {
    static constexpr int NLD = Nld<XW>::v, LD = XW + 4, XQ = XW / 4, KSTEP = NTHREADS / XQ;
    const float* colp;   // src + x  (nullptr if x beyond X)
    const int* gather;
    int ld, x;
    __device__ __forceinline__ void init(const float* src, int ld_, int X, int x0, const int* gather_, int tid) {
        ld = ld_;
        gather = gather_;
        x = x0 + 4 * (tid % XQ);
        colp = (x < X) ? src + x : nullptr;
    }
    __device__ __forceinline__ void load(float4 (&r)[NLD], int k0, int kend, int tid) const {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            int k = k0 + (tid / XQ) + KSTEP * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (colp != nullptr && k < kend) {
                long long row = gather ? (long long)gather[k] : (long long)k;
                v = *reinterpret_cast<const float4*>(colp + row * ld);
            }
            r[i] = v;
        }
    }
    __device__ __forceinline__ void store(float* lds, const float4 (&r)[NLD], int tid) const {
        float* base = lds + (tid / XQ) * LD + 4 * (tid % XQ);
#pragma unroll
        for (int i = 0; i < NLD; ++i) *reinterpret_cast<float4*>(base + KSTEP * i * LD) = r[i];
    }
};

template <int MODE, int XW> struct Loader;
template <int XW> struct Loader<OP_KC, XW> : KcLoader<XW> {
    __device__ __forceinline__ void fetch(float4 (&r)[Nld<XW>::v], int k0, int kend, int) const { this->load(r, k0, kend); }
};
template <int XW> struct Loader<OP_XC, XW> : XcLoader<XW> {
    __device__ __forceinline__ void fetch(float4 (&r)[Nld<XW>::v], int k0, int kend, int tid) const { this->load(r, k0, kend, tid); }
};

// ---- epilogue shared by both kernels.  MFMA 32x32 C/D layout: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5): a
// lane holds single floats of 16 rows.  Each wave transposes its 64x64 sub-tile through its own slice of the (now
// idle) pipeline LDS, 32 rows at a time, and stores 16-byte row segments: 16 store instructions per lane
// instead of 64 (the store tail of a short-K GEMM is issue bound).
// the 64 x 64 sub-tile whose first row / column is mrow0 / ncol0, staged through the wave-private slice `ep` (32 x 68 floats);
// wn = which 64-column half of its 128-column tile tn this is (the forward-only cross entropy's partials are per half)
// sum / maximum over the 16 lanes of a DPP row (every lane gets the result): quad xor 1, quad xor 2, row_half_mirror, row_mirror.
// (__shfl_xor(v, o, 16) is a ds_bpermute -- an LDS-path instruction with its own wait -- per step: four to eight of them in
// each of a tile's 32 store passes cost the fused-softmax projection 12 % of its tile time.)
#define FSMG_ROW16(OP)                                                                                          \
    v = OP(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true)));        \
    v = OP(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, true)));        \
    v = OP(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, true)));       \
    v = OP(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, true)));
// lane J of the own DPP row of 16 (row_newbcast:J)
template <int J> __device__ __forceinline__ float cs_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + J, 0xF, 0xF, true));
}
__device__ __forceinline__ float row16_add_(float a, float b) { return a + b; }
__device__ __forceinline__ float row16_sum(float v) { FSMG_ROW16(row16_add_) return v; }
__device__ __forceinline__ float row16_max(float v) { FSMG_ROW16(fmaxf) return v; }
#undef FSMG_ROW16

// The epilogue's mode is a compile-time property of the kernel (EM): one path per instantiation, chosen by launch_t from GemmArgs
// (ce_part / ce_store) exactly as the run-time branches used to choose it.
enum { EPI_PLAIN = 0, EPI_CE_FWD = 1, EPI_CE_STORE = 2 };   // plain store / forward-only cross entropy / fused softmax (ce_store)

// The bias of a lane's four columns.  They are the same in every store pass of a block tile (col = ncol0 + 4 * (lane & 15)), but the
// compiler may not hoist the load out of the passes itself -- the stores to C in between might alias g.bias -- and on this ISA a load
// per pass means a `s_waitcnt vmcnt(0)` per pass, which waits for the previous pass's STORES as well (vmcnt counts both).  So: one
// load per block tile, behind the k loop (no live range across it), and its wait paid here, once, in front of the first pass.
// `add` keeps the add conditional as it always was (col < N; z == 0 in the plain path): adding a zero would turn -0.0 into +0.0.
struct EpiBias { float4 v; bool add; };
template <int EM>
__device__ __forceinline__ EpiBias epi_bias(const GemmArgs& g, int z, int ncol0, int lane) {
    const int col = ncol0 + 4 * (lane & 15);
    EpiBias b;
    b.v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    b.add = g.bias != nullptr && col < g.N && (EM != EPI_PLAIN || z == 0);
    if (b.add) b.v = *reinterpret_cast<const float4*>(g.bias + col);
    __builtin_amdgcn_s_waitcnt(0x0f70);                        // vmcnt(0): the bias is here; no store pass waits on memory again
    return b;
}

template <int EM>
__device__ __forceinline__ void store_tile_at(const GemmArgs& g, f32x16 (&acc)[2][2], float* ep, int z, int mrow0, int ncol0,
                                              int tn, int tilesN, int wn, int lane, const EpiBias& bias) {
    const int l31 = lane & 31, khalf = lane >> 5;
    float* C = g.C + (long long)z * g.c_slab;
    constexpr int EP_LD = 68;                                  // 64 + 4: rows stay 16-byte aligned
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int tg[8];                                             // forward-only cross entropy: the targets of this lane's eight rows, loaded
        if constexpr (EM == EPI_CE_FWD) {                      // together ahead of the transpose (one load latency, not one per pass)
#pragma unroll
            for (int p = 0; p < 8; ++p) { const int row = mrow0 + i * 32 + p * 4 + (lane >> 4); tg[p] = row < g.M ? g.ce_tgt[row] : -1; }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ep[((r & 3) + 8 * (r >> 2) + 4 * khalf) * EP_LD + j * 32 + l31] = acc[i][j][r];
        // lgkmcnt(0): own LDS writes landed (wave-private slice); forward-only cross entropy: vmcnt(0) too -- the eight targets are
        // waited for here, once per block of passes, not at their first use inside a pass
        __builtin_amdgcn_s_waitcnt(EM == EPI_CE_FWD ? 0x0070 : 0xc07f);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int rl = p * 4 + (lane >> 4), c4 = (lane & 15) * 4;
            const int row = mrow0 + i * 32 + rl, col = ncol0 + c4;
            float4 v = *reinterpret_cast<const float4*>(ep + rl * EP_LD + c4);
            if (bias.add) { v.x += bias.v.x; v.y += bias.v.y; v.z += bias.v.z; v.w += bias.v.w; }
            if constexpr (EM == EPI_CE_STORE) {
                // train pass, fused softmax (GemmArgs::ce_store): E = exp(x) with NO shift into C (zero in the pad columns) and the sum of
                // the wave's 64 columns as this row's partial -- no row maximum, no target lookup (a dependent global load per pass cost
                // 14 % of the tile): k_ce_finish range-checks the row SUM and takes the target logit as log(E[target])
                float4 e;
                e.x = (col + 0 < g.ce_nvocab) ? __expf(v.x) : 0.0f; e.y = (col + 1 < g.ce_nvocab) ? __expf(v.y) : 0.0f;
                e.z = (col + 2 < g.ce_nvocab) ? __expf(v.z) : 0.0f; e.w = (col + 3 < g.ce_nvocab) ? __expf(v.w) : 0.0f;
                float sm = (e.x + e.y) + (e.z + e.w);
                sm = row16_sum(sm);
                if (row < g.M) {
                    if ((lane & 15) == 0) g.ce_part[(long long)row * (2 * tilesN) + 2 * tn + wn] = make_float2(0.0f, sm);
                    if (col < g.N) {
                        float* dst = C + (long long)row * g.ldc + col;
                        __builtin_nontemporal_store(e.x, dst); __builtin_nontemporal_store(e.y, dst + 1);
                        __builtin_nontemporal_store(e.z, dst + 2); __builtin_nontemporal_store(e.w, dst + 3);
                    }
                }
            } else if constexpr (EM == EPI_CE_FWD) {
                // forward-only cross entropy: softmax statistics of this row over the wave's 64 columns; the 16
                // lanes of a row (lane>>4 picks the row of this pass) reduce with width-16 shuffles
                const float NEG = -INFINITY;
                const float x0 = (col + 0 < g.ce_nvocab) ? v.x : NEG, x1 = (col + 1 < g.ce_nvocab) ? v.y : NEG;
                const float x2 = (col + 2 < g.ce_nvocab) ? v.z : NEG, x3 = (col + 3 < g.ce_nvocab) ? v.w : NEG;
                float m = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
                m = row16_max(m);
                float sm = 0.0f;
                if (m > NEG) sm = (expf(x0 - m) + expf(x1 - m)) + (expf(x2 - m) + expf(x3 - m));
                sm = row16_sum(sm);
                if (row < g.M) {
                    const int t = tg[p];
                    if (t >= col && t < col + 4) g.ce_tgt_logit[row] = (t == col) ? v.x : (t == col + 1) ? v.y : (t == col + 2) ? v.z : v.w;
                    if ((lane & 15) == 0) g.ce_part[(long long)row * (2 * tilesN) + 2 * tn + wn] = make_float2(m, sm);
                }
            } else {
                if (row < g.M && col < g.N) {                  // N, ldc are multiples of 4: whole float4 in or out
                    float4* dst = reinterpret_cast<float4*>(C + (long long)row * g.ldc + col);
                    if (g.nt_store) {   // write-once streaming output (logits): keep it out of the way of L2-resident data
                        __builtin_nontemporal_store(v.x, &dst->x); __builtin_nontemporal_store(v.y, &dst->y);
                        __builtin_nontemporal_store(v.z, &dst->z); __builtin_nontemporal_store(v.w, &dst->w);
                    } else {
                        *dst = v;
                    }
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);                    // reads done before the slice is overwritten
    }
}

template <int EM>
__device__ __forceinline__ void store_tile(const GemmArgs& g, f32x16 (&acc)[2][2], float* smem, int z, int m0, int n0,
                                           int tn, int tilesN, int wave, int lane) {
    const int wm = wave >> 1, wn = wave & 1;
    const EpiBias bias = epi_bias<EM>(g, z, n0 + wn * 64, lane);
    store_tile_at<EM>(g, acc, smem + wave * (32 * 68), z, m0 + wm * 64, n0 + wn * 64, tn, tilesN, wn, lane, bias);   // one 8.5 KiB slice per wave
}

// the fp32-MFMA kernels (k_gemm, k_gemm_staged, k_gemm_queue) keep the mode a run-time property, all three modes as before (a work-queue
// launch with bx3 = 1 or 2 runs k_gemm_queue whatever bx3 says, ce_store included): one branch in front of the passes
__device__ __forceinline__ void store_tile_rt(const GemmArgs& g, f32x16 (&acc)[2][2], float* smem, int z, int m0, int n0,
                                              int tn, int tilesN, int wave, int lane) {
    if (g.ce_part != nullptr && g.ce_store) store_tile<EPI_CE_STORE>(g, acc, smem, z, m0, n0, tn, tilesN, wave, lane);
    else if (g.ce_part != nullptr) store_tile<EPI_CE_FWD>(g, acc, smem, z, m0, n0, tn, tilesN, wave, lane);
    else store_tile<EPI_PLAIN>(g, acc, smem, z, m0, n0, tn, tilesN, wave, lane);
}

// XCD-aware tile numbering (bijective for any tile count): block b runs on XCD b % 8; each XCD walks a contiguous
// range of tiles, M fastest, so the blocks sharing a B panel sit in one L2
__device__ __forceinline__ int xcd_tile(int bid, int nb) {
    const int xcd = bid & 7, q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

// tile id (in the order an XCD walks its range) -> (row tile, column tile).  group_m = 0: row tiles fastest (a column
// panel of B is shared by consecutive blocks, A is streamed once per column panel).  group_m = G > 0: super-rows of G row
// tiles, inside a super-row column tiles slowest... i.e. G consecutive ids share a B panel and the next G the same A
// panels: the blocks resident on an XCD at one time then touch few panels of EITHER operand, so both stay in its 4 MiB L2
// (G = 1: column tiles fastest, for GEMMs whose A is the big operand).  Placement only; results do not change.
__device__ __forceinline__ void tile_coords(int t, int tilesM, int tilesN, int group_m, int& tm, int& tn) {
    if (group_m <= 0) { tm = t % tilesM; tn = t / tilesM; return; }
    const int per = group_m * tilesN;
    const int r = t / per, w = t - r * per;
    const int gm = min(group_m, tilesM - r * group_m);
    tn = w / gm;
    tm = r * group_m + (w - tn * gm);
}

template <int AMODE, int BMODE>
__global__ __launch_bounds__(NTHREADS, (BK == 16 ? 1024 : 512) / NTHREADS) void k_gemm_staged(const GemmArgs g) {
    constexpr int LDA = TileLd<AMODE, BM>::v, LDB = TileLd<BMODE, BN>::v;
    constexpr int ASZ = BK * LDA, BSZ = BK * LDB;
    constexpr int PIPE = 2 * ASZ + 2 * BSZ, EPI = NWAVES * 32 * 68;
    __shared__ __attribute__((aligned(16))) float smem[PIPE > EPI ? PIPE : EPI];
    float* As = smem;
    float* Bs = smem + 2 * ASZ;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, khalf = lane >> 5;

    // ---- XCD-aware tile numbering (bijective for any tile count)
    const int tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN;
    const int nb = tilesM * tilesN;
    const int bid = xcd_tile(blockIdx.x, nb);
    const int tm = bid % tilesM, tn = bid / tilesM;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- K range of this split
    const int z = blockIdx.y;
    int kb = 0, ke = g.K;
    if (g.ksplit > 1) {
        int per = ((g.K + g.ksplit - 1) / g.ksplit + BK - 1) / BK * BK;
        kb = z * per;
        ke = min(g.K, kb + per);
    }
    const int nk = (ke > kb) ? (ke - kb + BK - 1) / BK : 0;

    Loader<AMODE, BM> la;
    Loader<BMODE, BN> lb;
    la.init(g.A, g.lda, g.M, m0, g.gather, tid);
    lb.init(g.B, g.ldb, g.N, n0, nullptr, tid);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const bool do_colsum = (BMODE == OP_XC) && g.colsum != nullptr && tm == 0 && tid < BN;
    float csum = 0.0f;

    float4 ra[Nld<BM>::v], rb[Nld<BN>::v];
    if (nk > 0) {
        la.fetch(ra, kb, ke, tid);
        lb.fetch(rb, kb, ke, tid);
        la.store(As, ra, tid);
        lb.store(Bs, rb, tid);
    }
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            la.fetch(ra, kb + (kt + 1) * BK, ke, tid);
            lb.fetch(rb, kb + (kt + 1) * BK, ke, tid);
        }
        const float* a_base = As + cur * ASZ + khalf * LDA + wm * 64 + l31;
        const float* b_base = Bs + cur * BSZ + khalf * LDB + wn * 64 + l31;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float a0 = a_base[kk * LDA], a1 = a_base[kk * LDA + 32];
            const float b0 = b_base[kk * LDB], b1 = b_base[kk * LDB + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (do_colsum) {
            const float* bc = Bs + cur * BSZ + tid;
#pragma unroll
            for (int k = 0; k < BK; ++k) csum += bc[k * LDB];
        }
        if (more) {
            la.store(As + (cur ^ 1) * ASZ, ra, tid);
            lb.store(Bs + (cur ^ 1) * BSZ, rb, tid);
        }
        __syncthreads();
    }

    store_tile_rt(g, acc, smem, z, m0, n0, tn, tilesN, wave, lane);
    if (do_colsum && n0 + tid < g.N) g.colsum[(long long)z * g.colsum_slab + n0 + tid] = csum;
}

// ================================================================ main kernel
// LDS images (dense, 8 KiB per 128 x 16 operand tile, "lane-linear": wave w owns pieces 2w and 2w+1 of each tile,
// a piece is 1 KiB, and lane l's 16 bytes sit at piece + 16*l, so every ds_write_b128 is conflict free):
//   XC tile: [16 k][128 x] (rows of 512 B).  Piece p = rows 2p, 2p+1; lane -> row 2p + lane/32, x = 4*(lane%32).
//            MFMA operand read = ds_read_b32 at [k][x]: the two 32-lane halves read different rows and never
//            conflict (ds_read_b32 is serviced per half).
//   KC tile: 16-byte slots S = 4x + r; slot (x, r) holds k = 4*kq .. 4*kq+3 of row x with r = (kq + x/4) % 4.
//            Piece p = rows 16p .. 16p+15; lane -> x = 16p + lane/4, r = lane%4: the 4 lanes of a row fetch its 64
//            contiguous bytes (in rotated order) and store them untransposed.  MFMA operand read = one ds_read_b128
//            per 4 MFMAs; the rotation spreads each of that instruction's 16-lane groups over all 64 banks.
// K order inside a tile: a ds_read_b128 hands a lane four consecutive k of one row, so MFMA (jj, j), j = 0..3,
// contracts k = 4*(2*jj + half) + j (half = lane/32) instead of k = 2*step + half; both operands follow the same
// convention in either storage mode, and a sum over k does not care about the order it is taken in.
// Edges: rows/columns past M or N are clamped to the last valid one (their products land in output rows/columns
// that are never stored), so the steady-state loop has no predicated loads; a K range that is not a multiple of 16
// zero-fills its last tile.
// Global loads for tile t+1 are issued before the MFMAs of tile t (register prefetch) and written to the other LDS
// buffer afterwards: one barrier per K tile.  (LDS-DMA, global_load_lds_dwordx4 into the same images, was measured
// 5-10 % slower than this at 4 pieces per wave and tile: DESIGN.md "rejected".)
constexpr int TILE_F = 128 * BK;        // floats per operand tile (both layouts are dense)
constexpr int PIECE_F = 256;            // floats per wave instruction (1 KiB)

template <int MODE>
struct Stager {
    const float* p[2];
    float4 r[2];
    long long step;
    int kofs[2];
    __device__ __forceinline__ void init(const float* src, int ld, int X, int x0, const int* gather, int kb, int wave, int lane) {
        if (MODE == OP_XC) {
            int x = x0 + 4 * (lane & 31);
            x = min(x, X - 4);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                kofs[i] = 4 * wave + 2 * i + (lane >> 5);
                p[i] = src + (long long)(kb + kofs[i]) * ld + x;
            }
            step = (long long)BK * ld;
        } else {
            const int xi = lane >> 2, r = lane & 3;
            const int kq = (r - (xi >> 2)) & 3;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int x = x0 + 16 * (2 * wave + i) + xi;
                x = min(x, X - 1);
                const long long row = gather ? (long long)gather[x] : (long long)x;
                kofs[i] = 4 * kq;
                p[i] = src + row * ld + kb + 4 * kq;
            }
            step = BK;
        }
    }
    // full tile: unconditional 16-byte loads now ...
    __device__ __forceinline__ void fetch() {
#pragma unroll
        for (int i = 0; i < 2; ++i) { r[i] = *reinterpret_cast<const float4*>(p[i]); p[i] += step; }
    }
    // ... LDS writes after the MFMAs of the current tile
    __device__ __forceinline__ void commit(float* tile, int wave, int lane) const {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(tile + (2 * wave + i) * PIECE_F + 4 * lane) = r[i];
    }
    // partial tile (k0 + 16 > kend): zeros past kend
    __device__ __forceinline__ void fetch_partial(int k0, int kend) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            r[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + kofs[i] < kend) r[i] = *reinterpret_cast<const float4*>(p[i]);
            p[i] += step;
        }
    }
};

// the four operand values of lane (x, half) for MFMAs (jj, 0..3)
template <int MODE>
__device__ __forceinline__ void read_frag(const float* tile, int x, int half, int jj, float (&f)[4]) {
    if (MODE == OP_KC) {
        const int kq = 2 * jj + half;
        const float4 v = *reinterpret_cast<const float4*>(tile + 4 * (4 * x + ((kq + (x >> 2)) & 3)));
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else {
        const float* r = tile + (4 * (2 * jj + half)) * 128 + x;
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = r[j * 128];
    }
}

// one 128 x 128 tile of split z: the body shared by the static-grid kernel and the work-queue kernel below
template <int AMODE, int BMODE>
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, float* smem, int tm, int tn, int z, int tilesN) {
    constexpr int TILE_F_ = TILE_F;
    float* As = smem;                   // [2][TILE_F]
    float* Bs = smem + 2 * TILE_F_;     // [2][TILE_F]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, khalf = lane >> 5;
    const int m0 = tm * 128, n0 = tn * 128;

    int kb = 0, ke = g.K;
    if (g.ksplit > 1) {
        const int per = ((g.K + g.ksplit - 1) / g.ksplit + BK - 1) / BK * BK;
        kb = z * per;
        ke = min(g.K, kb + per);
    }
    const int nk = (ke > kb) ? (ke - kb + BK - 1) / BK : 0;
    const int nfull = (ke > kb) ? (ke - kb) / BK : 0;

    Stager<AMODE> sa;
    Stager<BMODE> sb;
    sa.init(g.A, g.lda, g.M, m0, g.gather, kb, wave, lane);
    sb.init(g.B, g.ldb, g.N, n0, nullptr, kb, wave, lane);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const bool do_colsum = (BMODE == OP_XC) && g.colsum != nullptr && tm == 0 && tid < 128;
    float csum = 0.0f;

    if (nk > 0) {
        if (nfull > 0) { sa.fetch(); sb.fetch(); }
        else { sa.fetch_partial(kb, ke); sb.fetch_partial(kb, ke); }
        sa.commit(As, wave, lane);
        sb.commit(Bs, wave, lane);
    }
    __syncthreads();

    const int xa = wm * 64 + l31, xb = wn * 64 + l31;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            if (kt + 1 < nfull) { sa.fetch(); sb.fetch(); }
            else { sa.fetch_partial(kb + (kt + 1) * BK, ke); sb.fetch_partial(kb + (kt + 1) * BK, ke); }
        }
        const float* at = As + cur * TILE_F_;
        const float* bt = Bs + cur * TILE_F_;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            float a0[4], a1[4], b0[4], b1[4];
            read_frag<AMODE>(at, xa, khalf, jj, a0);
            read_frag<AMODE>(at, xa + 32, khalf, jj, a1);
            read_frag<BMODE>(bt, xb, khalf, jj, b0);
            read_frag<BMODE>(bt, xb + 32, khalf, jj, b1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc[1][1], 0, 0, 0);
            }
        }
        if (do_colsum) {
            const float* bc = bt + tid;
#pragma unroll
            for (int k = 0; k < BK; ++k) csum += bc[k * 128];
        }
        if (more) {
            sa.commit(As + (cur ^ 1) * TILE_F_, wave, lane);
            sb.commit(Bs + (cur ^ 1) * TILE_F_, wave, lane);
        }
        __syncthreads();
    }

    store_tile_rt(g, acc, smem, z, m0, n0, tn, tilesN, wave, lane);
    if (do_colsum && n0 + tid < g.N) g.colsum[(long long)z * g.colsum_slab + n0 + tid] = csum;
}

template <int AMODE, int BMODE>
__global__ __launch_bounds__(256, 4) void k_gemm(const GemmArgs g) {
    static_assert(BK == 16 && BM == 128, "the direct-to-LDS kernel is written for 128x128x16 tiles");
    constexpr int PIPE = 4 * TILE_F, EPI = 4 * 32 * 68;
    __shared__ __attribute__((aligned(1024))) float smem[PIPE > EPI ? PIPE : EPI];
    const int tilesM = (g.M + 127) / 128, tilesN = (g.N + 127) / 128;
    const int bid = xcd_tile(blockIdx.x, tilesM * tilesN);
    gemm_tile<AMODE, BMODE>(g, smem, bid % tilesM, bid / tilesM, blockIdx.y, tilesN);
}

// Work-queue variant for the XCD-partitioned schedule (GemmArgs::xcd_first): every block draws ONE (split, row tile,
// column tile) item, row tiles slowest, in the order blocks start -- so XCDs that are busy with something else simply
// draw fewer.  A restricted launch
// (xcd_first > 0) only lets blocks on XCDs >= xcd_first draw, and only while *stop == 0 and below work_limit items; the
// clean-up launch (xcd_first < 0) drains the queue chip-wide.  Which block computes a tile never changes the tile.
template <int AMODE, int BMODE>
__global__ __launch_bounds__(256, 4) void k_gemm_queue(const GemmArgs g) {
    constexpr int PIPE = 4 * TILE_F, EPI = 4 * 32 * 68;
    __shared__ __attribute__((aligned(1024))) float smem[PIPE > EPI ? PIPE : EPI];
    __shared__ int s_item;
    const int tilesM = (g.M + 127) / 128, tilesN = (g.N + 127) / 128;
    const int total = tilesM * tilesN * (g.ksplit > 1 ? g.ksplit : 1);
    const int limit = g.xcd_first > 0 ? min(g.work_limit, total) : total;
    if (g.xcd_first > 0) {
        int xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if ((xcc & 7) < g.xcd_first) return;
    }
    if (threadIdx.x == 0) {
        // one atomicAdd per block (a CAS loop on the counter serialises the whole chip at ~2 us per item); the per-item
        // claim word settles restricted launch against clean-up launch
        int item = -1;
        if (g.xcd_first < 0) {
            const int j = atomicAdd(g.work + 1, 1);
            if (j < total && atomicCAS(g.claim + j, 0, 1) == 0) item = j;
        } else if (__hip_atomic_load(g.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
            const int j = atomicAdd(g.work, 1);
            if (j < limit && atomicCAS(g.claim + j, 0, 1) == 0) item = j;
        }
        s_item = item;
    }
    __syncthreads();
    const int item = s_item;
    if (item < 0) return;
    gemm_tile<AMODE, BMODE>(g, smem, (item / tilesN) % tilesM, item % tilesN, item / (tilesM * tilesN), tilesN);
}

// ---------------------------------------------------------------------------------------------------------------
// fp32 GEMM on the bf16 matrix pipe ("bx3"): v_mfma_f32_32x32x16_bf16 runs at 16x the rate of the fp32 MFMA, so an
// fp32 product is assembled from bf16 pieces.  Every operand value is split EXACTLY into three bf16 numbers
//     a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)
// (round-to-nearest: |a2| <= 2^-8 |a|, |a3| <= 2^-16 |a|, and the last residual fits 8 significant bits; the two
// subtractions are exact in fp32), and the six partial products that matter are accumulated in fp32:
//     a b ~= a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a3 b1 + a2 b2),   dropped: a2 b3 + a3 b2 + a3 b3 <= 2^-23 |a b|
// i.e. one half-ulp of the fp32 product, unbiased -- the accumulation (fp32, as in the fp32 MFMA) dominates the error
// either way.  6 MFMAs of 32x32x16 (32 cycles each) replace 8 of 32x32x2 (64 cycles each) per 16 k: 2.67x the rate.
// (Finite inputs, that is -- values above bf16's largest, 3.39e38, included: measured finite.  An Inf operand makes the
// second piece NaN (bf16(Inf - Inf)) and the products it feeds NaN where the fp32 MFMA produces Inf; pinned by
// tests/test_gpu_parity.py::test_non_finite_weights_give_nan_...; NaN inputs give NaN in both.)
// The split runs on the VALU between the global load and the LDS write (5.5 instructions per element), the LDS holds
// the three planes as [plane][k half][128 x][8 bf16] so that a fragment is one conflict-free ds_read_b128 per lane.
// Same tiling, epilogue, split-K and XCD-aware tile order as k_gemm; same A / B conventions.
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8_t;

__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
}
// two fp32 values -> their three bf16 planes, packed (x in the low half)
__device__ __forceinline__ void split2(float x, float y, unsigned& p0, unsigned& p1, unsigned& p2) {
    p0 = cvt_pk_bf16(x, y);
    const float rx = x - __uint_as_float(p0 << 16), ry = y - __uint_as_float(p0 & 0xffff0000u);
    p1 = cvt_pk_bf16(rx, ry);
    const float sx = rx - __uint_as_float(p1 << 16), sy = ry - __uint_as_float(p1 & 0xffff0000u);
    p2 = cvt_pk_bf16(sx, sy);
}

// the same for eight values, the four independent chains advanced stage by stage: the instructions of one chain depend on
// each other (a wave alone needs 62 cycles per pair that way, tools/split_probe), and the compiler keeps inline asm in
// source order, so the interleaving is written out
__device__ __forceinline__ float sub_f32(float a, unsigned b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ void split8(const float (&v)[8], unsigned (&w)[3][4]) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[0][j] = cvt_pk_bf16(v[2 * j], v[2 * j + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[2 * j] = sub_f32(v[2 * j], w[0][j] << 16); r[2 * j + 1] = sub_f32(v[2 * j + 1], w[0][j] & 0xffff0000u); }
#pragma unroll
    for (int j = 0; j < 4; ++j) w[1][j] = cvt_pk_bf16(r[2 * j], r[2 * j + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[2 * j] = sub_f32(r[2 * j], w[1][j] << 16); r[2 * j + 1] = sub_f32(r[2 * j + 1], w[1][j] & 0xffff0000u); }
#pragma unroll
    for (int j = 0; j < 4; ++j) w[2][j] = cvt_pk_bf16(r[2 * j], r[2 * j + 1]);
}

constexpr int BX_PLANE = 2 * 128 * 16;          // bytes: [2 k halves][128 x][8 bf16]
constexpr int BX_OPER = 3 * BX_PLANE;           // one operand tile, three planes
constexpr int BX_STAGE = 2 * BX_OPER;           // A + B

// Global -> registers -> LDS for one operand tile (128 x, 16 k).  Eight values per thread either way:
//   XC (x contiguous): thread = (x = tid % 128, k half = tid / 128), eight 4-byte loads down k (a wave reads 256
//       contiguous bytes per load); one 16-byte LDS write per plane;
//   KC (k contiguous): thread = (rows tid / 4 and tid / 4 + 64, k quad = tid % 4), two 16-byte loads (four lanes cover
//       the 64 bytes a row contributes to the tile); two 8-byte LDS writes per plane.
//   XC with gathered K rows (dKx: row k of the operand is row gather[k] of the embedding): the eight row ids of the NEXT
//       tile are fetched one tile ahead, so a tile's loads do not wait for an index load first.
template <int MODE, int XT = 128, int NT = 256, bool BUF = false>   // XT: x extent of the LDS tile written into; NT threads cover NT / 2 of them
struct BxStager {
    static constexpr int KH = XT * 16, PLANE = 2 * KH, XW = NT / 2;
    const float* p[2];
    const float* src_;
    float v[8];
    long long step, ld_;
    int lds_ofs[2];
    const int* gp;          // XC + gather: &gather[k] of this thread's first row of the next tile
    int gk, gK;             // ... that k, and the K bound of the gather array
    int gi[8];
    int kstep;              // k advance per fetch: 16, or 32 when two stagers take alternate tiles (k_gemm_bx3w)
    // Buffer loads (SGPR base + 32-bit lane offset + SGPR k offset) instead of 64-bit lane addresses wherever the operand
    // fits 4 GiB and has no gathered K rows: the eight 4-byte loads of an x-contiguous tile then need no per-load address
    // arithmetic on the VALU (a loader wave of k_gemm_bx3w issues them in 590 cycles instead of 1650 with all loads hitting
    // the L1, profiles/r03_gemm_buf1.log; dW 0.435 -> 0.397 ms, dKh 0.094 -> 0.085, the projection 0.335 -> 0.302)
    // (BUF is the launcher's decision: launch_t checks the sizes and the gather)
    __amdgpu_buffer_rsrc_t rs;
    unsigned vo[2], so, sstep;
    static constexpr bool use_buf = BUF;
    __device__ __forceinline__ void load_ids() {
#pragma unroll
        for (int i = 0; i < 8; ++i) gi[i] = gp[min(i, gK - 1 - gk)];      // clamped: the id of a row past K is never used
    }
    __device__ __forceinline__ void init(const float* src, int ld, int X, int x0, const int* gather, int kb, int tid, int K = 0, int kstep_ = 16, int xl0 = 0) {
        ld_ = ld; gp = nullptr; kstep = kstep_;
        if (MODE == OP_XC) {
            const int x = min(x0 + (tid % XW), X - 1), kh = tid / XW;
            p[0] = src + (long long)(kb + 8 * kh) * ld + x; p[1] = nullptr;
            step = (long long)kstep * ld;
            lds_ofs[0] = kh * KH + (xl0 + (tid % XW)) * 16; lds_ofs[1] = 0;
            if (gather != nullptr) {
                p[0] = src + x;
                gK = K; gk = min(kb + 8 * kh, K - 1); gp = gather + gk;
                load_ids();
            }
        } else {
            const int kq = tid & 3;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int xl = (tid >> 2) + (NT / 4) * i, x = min(x0 + xl, X - 1);
                const long long row = gather ? (long long)gather[x] : (long long)x;
                p[i] = src + row * ld + kb + 4 * kq;
                lds_ofs[i] = (kq >> 1) * KH + (xl0 + xl) * 16 + (kq & 1) * 8;
            }
            step = kstep;
        }
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)0xfffffffcu, 0x00020000);
        so = 0; sstep = (unsigned)(step * 4);
        vo[0] = (unsigned)((p[0] - src) * 4);
        vo[1] = (MODE == OP_XC) ? 0u : (unsigned)((p[1] - src) * 4);
        src_ = src;            // (buffer-load path: the lane pointers p[] are not kept, the K tail rebuilds them from vo[])
    }
    __device__ __forceinline__ void advance_ids() {          // ids of the tile after the one just requested
        const int nk = min(gk + kstep, gK - 1);
        gp += nk - gk; gk = nk;
        load_ids();
    }
    __device__ __forceinline__ void fetch() {
        if (MODE == OP_XC) {
            if (gp != nullptr) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = p[0][(long long)gi[i] * ld_];
                advance_ids();
                return;
            }
            if (use_buf) {
                const unsigned s0 = __builtin_amdgcn_readfirstlane(so), ldb = (unsigned)ld_ * 4;
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, vo[0], s0 + i * ldb, 0));
                so += sstep;                // (p stays at the K range's start: fetch_partial adds `so`)
                return;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = p[0][i * ld_];
            p[0] += step;
        } else {
            if (use_buf) {
                typedef unsigned u4_ __attribute__((ext_vector_type(4)));
                const unsigned s0 = __builtin_amdgcn_readfirstlane(so);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const u4_ q = __builtin_amdgcn_raw_buffer_load_b128(rs, vo[i], s0, 0);
                    v[4 * i] = __uint_as_float(q.x); v[4 * i + 1] = __uint_as_float(q.y); v[4 * i + 2] = __uint_as_float(q.z); v[4 * i + 3] = __uint_as_float(q.w);
                }
                so += sstep;
                return;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 q = *reinterpret_cast<const float4*>(p[i]);
                v[4 * i] = q.x; v[4 * i + 1] = q.y; v[4 * i + 2] = q.z; v[4 * i + 3] = q.w;
                p[i] += step;
            }
        }
    }
    // last tile of a K range: k0 = first k of the tile, zeros from kend on
    __device__ __forceinline__ void fetch_partial(int k0, int kend, int tid) {
        const long long adv = use_buf ? (long long)(so >> 2) : 0;      // buffer-load path: the pointers never moved
        so += sstep;
        if (MODE == OP_XC) {
            const int kh = tid / XW;
            if (gp != nullptr) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (k0 + 8 * kh + i < kend) ? p[0][(long long)gi[i] * ld_] : 0.0f;
                advance_ids();
                return;
            }
            const float* q = use_buf ? src_ + (vo[0] >> 2) + adv : p[0];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (k0 + 8 * kh + i < kend) ? q[i * ld_] : 0.0f;
            if (!use_buf) p[0] += step;
        } else {
            const int kq = tid & 3;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* q = use_buf ? src_ + (vo[i] >> 2) + adv : p[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * i + e] = (k0 + 4 * kq + e < kend) ? q[e] : 0.0f;
                if (!use_buf) p[i] += step;
            }
        }
    }
    __device__ __forceinline__ void load() {}                 // (the values are in registers once the loads have landed)
    __device__ __forceinline__ float sum8() const { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }
    __device__ __forceinline__ void commit(unsigned char* tile) const {
        unsigned w[3][4];
        split8(v, w);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            if (MODE == OP_XC) {
                *reinterpret_cast<uint4*>(tile + pl * PLANE + lds_ofs[0]) = make_uint4(w[pl][0], w[pl][1], w[pl][2], w[pl][3]);
            } else {
                *reinterpret_cast<uint2*>(tile + pl * PLANE + lds_ofs[0]) = make_uint2(w[pl][0], w[pl][1]);
                *reinterpret_cast<uint2*>(tile + pl * PLANE + lds_ofs[1]) = make_uint2(w[pl][2], w[pl][3]);
            }
        }
    }
};

// An x-contiguous operand tile through LDS-DMA (k_gemm_bx3h, 512 threads, XT = 256): the register path above needs eight
// 4-byte loads per thread down k, and a CU takes one wave-level load per 16-26 cycles whatever its width -- 64 of the 80
// loads of a k tile carry 256 bytes each.  Here wave w owns columns 32 w ... 32 w + 31 of the tile: two
// `buffer_load_dwordx4 ... lds` per lane (lane = (k row % 8, x quad); eight k rows of 128 contiguous bytes per instruction)
// drop the raw fp32 block [16 k][32 x] into a 2 KiB LDS region of the wave's own, and the commit reads it back transposed
// (lane = (x, k half): eight ds_read_b32 down k, conflict-free), splits and writes the planes as before.  No other wave
// touches the region, so the only synchronisation is the wave's own vmcnt / lgkmcnt; the prefetched tile costs no registers.
// Needs ld % 4 == 0, X % 4 == 0, a 16-byte aligned base and the operand below 4 GiB (launch_t checks).
typedef __attribute__((address_space(3))) void* bx_lds_ptr_t;
template <int XT, bool GATHER = false>
struct BxDmaXC {
    static constexpr int KH = XT * 16, PLANE = 2 * KH;
    __amdgpu_buffer_rsrc_t rs;
    unsigned vo[2], so, sstep, ldb;
    unsigned char* raw;        // the wave's 2 KiB region (wave-uniform)
    int rd_ofs, lds_ofs, kvalid;
    float v[8];
    // GATHER (the two-part A of GemmArgs::m_split): row k of the operand is row gidx[k] of the table (gidx == nullptr: row k).  The row
    // ids of the NEXT tile are requested right behind this tile's DMA loads and are in by the time the following fetch() needs them
    // (load()'s vmcnt(0) sits in between); rows past the K range are clamped to its last row here and zeroed in load() as always.
    const int* gidx; int gk[2], gend; unsigned xofs, gnext[2];
    __device__ __forceinline__ unsigned grow(int i) { const int k = min(gk[i], gend); gk[i] += 16; return gidx ? (unsigned)gidx[k] : (unsigned)k; }
    __device__ __forceinline__ void init(const float* src, int ld, int X, int x0, const int* gather, int kb, int tid, int = 0, unsigned char* raw_ = nullptr, int kend = 0) {
        const int lane = tid & 63, wave = tid >> 6;
        raw = raw_;
        const int xcol = min(x0 + 32 * wave + 4 * (lane & 7), X - 4), krow = lane >> 3;
        ldb = (unsigned)ld * 4u;
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, (int)0xfffffffcu, 0x00020000);
        if constexpr (GATHER) {
            gidx = gather; gend = kend - 1; xofs = (unsigned)xcol * 4u;
#pragma unroll
            for (int i = 0; i < 2; ++i) gk[i] = kb + 8 * i + krow;
#pragma unroll
            for (int i = 0; i < 2; ++i) vo[i] = grow(i) * ldb + xofs;
#pragma unroll
            for (int i = 0; i < 2; ++i) gnext[i] = grow(i);
            so = 0; sstep = 0;
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) vo[i] = (unsigned)(kb + 8 * i + krow) * ldb + (unsigned)xcol * 4u;
            so = 0; sstep = 16u * ldb;
        }
        rd_ofs = ((lane >> 5) * 256 + (lane & 31)) * 4;
        lds_ofs = (lane >> 5) * KH + (32 * wave + (lane & 31)) * 16;
        kvalid = 16;
    }
    __device__ __forceinline__ void fetch() {
        const unsigned s0 = __builtin_amdgcn_readfirstlane(so);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (bx_lds_ptr_t)raw, 16, vo[0], s0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (bx_lds_ptr_t)(raw + 1024), 16, vo[1], s0, 0, 0);
        if constexpr (GATHER) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { vo[i] = gnext[i] * ldb + xofs; gnext[i] = grow(i); }
        } else {
            so += sstep;
        }
    }
    // last tile of a K range: rows from kend on are read from row kend - 1 and zeroed in load()
    __device__ __forceinline__ void fetch_partial(int k0, int kend, int tid) {
        if constexpr (GATHER) {
            fetch();                        // (clamped to row kend - 1 when the row ids were requested)
            kvalid = kend - k0;
            return;
        }
        const int krow = (tid & 63) >> 3;
#pragma unroll
        for (int i = 0; i < 2; ++i) {         // vo[i] + so addresses row k0 + 8 i + krow: step back to row kend - 1 from beyond it
            const int over = max(k0 + 8 * i + krow - (kend - 1), 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (bx_lds_ptr_t)(raw + 1024 * i), 16, vo[i] + so - (unsigned)over * ldb, 0, 0, 0);
        }
        so += sstep;
        kvalid = kend - k0;
    }
    __device__ __forceinline__ void load() {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float* r = reinterpret_cast<const float*>(raw + rd_ofs);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = r[j * 32];
        if (kvalid < 16) {
            const int khalf8 = (rd_ofs >> 10) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) if (khalf8 + j >= kvalid) v[j] = 0.0f;
        }
    }
    __device__ __forceinline__ float sum8() const { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }
    __device__ __forceinline__ void commit(unsigned char* tile) const {
        unsigned w[3][4];
        split8(v, w);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(tile + pl * PLANE + lds_ofs) = make_uint4(w[pl][0], w[pl][1], w[pl][2], w[pl][3]);
    }
};
template <bool DMA, int MODE, int XT, int NT, bool BUF, bool GATHER = false> struct BxStagerSel { typedef BxStager<MODE, XT, NT, BUF> type; };
template <int XT, int NT, bool BUF, bool GATHER> struct BxStagerSel<true, OP_XC, XT, NT, BUF, GATHER> { typedef BxDmaXC<XT, GATHER> type; };

// PROF (tools/gemm_bench PROF=1): per (block, wave) s_memtime stamps -> g.prof[(block * 4 + wave) * 8 + ...]:
//   [0] entry, [1] first loop iteration, [2] sum over k tiles of (fragment reads + MFMA issue), [3] sum of (wait for the
//   next tile's loads + split + LDS writes), [4] sum of (LDS drain + barrier), [5] loop exit, [6] kernel exit,
//   [7] XCC_ID << 32 | HW_ID
#define BX_STAMP(i) if (PROF) { __builtin_amdgcn_sched_barrier(0); const unsigned long long n_ = __builtin_amdgcn_s_memtime(); \
                                __builtin_amdgcn_sched_barrier(0); pacc[i] += n_ - plast; plast = n_; }
// BUFM: which operands are fetched with buffer loads (0 none, 1 B only, 2 both; BxStager)
// EM: the epilogue's mode (EPI_*), see store_tile_at
template <int AMODE, int BMODE, bool PROF = false, int BUFM = 0, int EM = EPI_PLAIN>
__global__ __launch_bounds__(256, 2) void k_gemm_bx3(const GemmArgs g) {
    constexpr int EPI = 4 * 32 * 68 * 4;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[(2 * BX_STAGE > EPI) ? 2 * BX_STAGE : EPI];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tilesM = (g.M + 127) / 128, tilesN = (g.N + 127) / 128;
    const int bid = xcd_tile(blockIdx.x, tilesM * tilesN);
    int tm, tn; tile_coords(bid, tilesM, tilesN, g.group_m, tm, tn);
    const int z = blockIdx.y;
    const int m0 = tm * 128, n0 = tn * 128;
    unsigned long long pacc[5] = {0, 0, 0, 0, 0}, plast = 0, p_entry = 0, p_loop = 0;
    if (PROF) { p_entry = plast = __builtin_amdgcn_s_memtime(); }

    int kb = 0, ke = g.K;
    if (g.ksplit > 1) {
        const int per = ((g.K + g.ksplit - 1) / g.ksplit + 15) / 16 * 16;
        kb = z * per;
        ke = min(g.K, kb + per);
    }
    const int nk = (ke > kb) ? (ke - kb + 15) / 16 : 0;
    const int nfull = (ke > kb) ? (ke - kb) / 16 : 0;

    BxStager<AMODE, 128, 256, (BUFM >= 2)> sa;
    BxStager<BMODE, 128, 256, (BUFM >= 1)> sb;
    sa.init(g.A, g.lda, g.M, m0, g.gather, kb, tid, g.K);
    sb.init(g.B, g.ldb, g.N, n0, nullptr, kb, tid, g.K);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const bool do_colsum = (BMODE == OP_XC) && g.colsum != nullptr && tm == 0;
    float csum = 0.0f;

    if (nk > 0) {
        if (nfull > 0) { sa.fetch(); sb.fetch(); }
        else { sa.fetch_partial(kb, ke, tid); sb.fetch_partial(kb, ke, tid); }
        if (do_colsum) csum += sb.sum8();
        sa.commit(smem);
        sb.commit(smem + BX_OPER);
    }
    __syncthreads();

    const int fa = khalf * 2048 + (wm * 64 + l31) * 16, fb = khalf * 2048 + (wn * 64 + l31) * 16;
    if (PROF) { p_loop = plast = __builtin_amdgcn_s_memtime(); }
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
            if (kt + 1 < nfull) { sa.fetch(); sb.fetch(); }
            else { sa.fetch_partial(kb + (kt + 1) * 16, ke, tid); sb.fetch_partial(kb + (kt + 1) * 16, ke, tid); }
        }
        const unsigned char* at = smem + cur * BX_STAGE;
        const unsigned char* bt = at + BX_OPER;
        bf16x8_t a[3][2], b[3][2];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[pl][i] = *reinterpret_cast<const bf16x8_t*>(at + pl * BX_PLANE + fa + i * 512);
                b[pl][i] = *reinterpret_cast<const bf16x8_t*>(bt + pl * BX_PLANE + fb + i * 512);
            }
        // smallest terms first; four independent accumulators per term keep the pipe full
#define BX_TERM(PA, PB)                                                                                        \
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][0], b[PB][0], acc[0][0], 0, 0, 0);            \
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][0], b[PB][1], acc[0][1], 0, 0, 0);            \
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][1], b[PB][0], acc[1][0], 0, 0, 0);            \
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][1], b[PB][1], acc[1][1], 0, 0, 0);
        BX_TERM(2, 0) BX_TERM(0, 2) BX_TERM(1, 1) BX_TERM(1, 0) BX_TERM(0, 1) BX_TERM(0, 0)
#undef BX_TERM
        BX_STAMP(2)
        if (more) {
            if (do_colsum) csum += sb.sum8();
            sa.commit(smem + (cur ^ 1) * BX_STAGE);
            sb.commit(smem + (cur ^ 1) * BX_STAGE + BX_OPER);
        }
        BX_STAMP(3)
        __syncthreads();
        BX_STAMP(4)
    }
    const unsigned long long p_exit_loop = PROF ? __builtin_amdgcn_s_memtime() : 0;

    float* smem_f = reinterpret_cast<float*>(smem);
    if (do_colsum) {                    // the two k halves of a column live in threads tid and tid + 128
        __shared__ float s_cs[128];
        if (tid >= 128) s_cs[tid - 128] = csum;
        __syncthreads();
        if (tid < 128 && n0 + tid < g.N) g.colsum[(long long)z * g.colsum_slab + n0 + tid] = csum + s_cs[tid];
    }
    store_tile<EM>(g, acc, smem_f, z, m0, n0, tn, tilesN, wave, lane);
    if (PROF && g.prof != nullptr && lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long p_end = __builtin_amdgcn_s_memtime();
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* o = g.prof + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 8;
        o[0] = p_entry; o[1] = p_loop; o[2] = pacc[2]; o[3] = pacc[3]; o[4] = pacc[4]; o[5] = p_exit_loop; o[6] = p_end;
        o[7] = ((unsigned long long)xcc << 32) | hw;
    }
}

// Wave-specialised variants (GemmArgs::bx3 == 2: MT = 1, 128 x 128 block tile; bx3 == 3: MT = 2, 256 x 128): the same LDS
// image per 128 rows, k order and term order as k_gemm_bx3 -- hence the same bits for the same K split -- but the block has
// 4 MT "multiplier" waves (64 x 64 each) that only read fragments and issue MFMAs, and 4 "loader" waves that only load, split
// and write the next tile (a workgroup's waves are dealt to the SIMDs cyclically, so every SIMD gets MT multipliers and one
// loader per block).  Why (tools/gemm_bench PROF=1, profiles/r03_gemm_prof*.log): in k_gemm_bx3 a lone 4-wave block needs
// 2470 cycles per k tile for 768 cycles of MFMAs -- reads, MFMAs, ~100 VALU instructions of the split, LDS writes and the
// barrier are one serial chain per wave, and three co-resident blocks only fill the matrix pipe to 70 %.  With the roles
// split the multipliers' chain is reads + MFMAs (1060-1300 cycles), and the split issues in the MFMA shadow of other waves;
// it then is the VALU that binds (31 cycles per value: 16 values per thread and k tile = 500 of the 768 cycles per multiplier
// wave at MT = 1), which is what MT = 2 relieves: a 256 x 128 tile splits 0.75 x the values per MFMA.
// The loaders fetch two tiles ahead (two register sets taking alternate tiles).
__device__ __forceinline__ void bx_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int AMODE, int BMODE, int MT, bool PROF = false, int BUFM = 0, int EM = EPI_PLAIN>
__global__ __launch_bounds__(256 * (MT + 1), MT == 1 ? 2 : 1) void k_gemm_bx3w(const GemmArgs g) {
    constexpr int XA = 128 * MT;                       // rows of the block tile
    constexpr int A_PLANE = 2 * XA * 16, A_OPER = 3 * A_PLANE, STAGE = A_OPER + BX_OPER;
    constexpr int EPI = 4 * MT * 32 * 68 * 4;
    constexpr int NMW = 4 * MT;                        // multiplier waves
    __shared__ __attribute__((aligned(1024))) unsigned char smem[(2 * STAGE > EPI) ? 2 * STAGE : EPI];
    __shared__ float s_cs[128];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tilesM = (g.M + XA - 1) / XA, tilesN = (g.N + 127) / 128;
    const int bid = xcd_tile(blockIdx.x, tilesM * tilesN);
    int tm, tn; tile_coords(bid, tilesM, tilesN, g.group_m, tm, tn);
    const int z = blockIdx.y;
    const int m0 = tm * XA, n0 = tn * 128;
    unsigned long long pacc[5] = {0, 0, 0, 0, 0}, plast = 0, p_entry = 0, p_loop = 0, p_exit_loop = 0;
    if (PROF) { p_entry = plast = __builtin_amdgcn_s_memtime(); }

    int kb = 0, ke = g.K;
    if (g.ksplit > 1) {
        const int per = ((g.K + g.ksplit - 1) / g.ksplit + 15) / 16 * 16;
        kb = z * per;
        ke = min(g.K, kb + per);
    }
    const int nk = (ke > kb) ? (ke - kb + 15) / 16 : 0;
    const int nfull = (ke > kb) ? (ke - kb) / 16 : 0;

    if (wave >= NMW) {
        // ---------------------------------------------------------------- loaders: tile kt + 1 is split and written while
        // the others multiply tile kt; its values were requested two iterations earlier
        const int lt = tid - 64 * NMW;
        BxStager<AMODE, XA, 256, (BUFM >= 2)> sa[2][MT];
        BxStager<BMODE, 128, 256, (BUFM >= 1)> sb[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int i = 0; i < MT; ++i) sa[q][i].init(g.A, g.lda, g.M, m0 + 128 * i, g.gather, kb + 16 * q, lt, g.K, 32, 128 * i);
            sb[q].init(g.B, g.ldb, g.N, n0, nullptr, kb + 16 * q, lt, g.K, 32);
        }
        if (PROF && (g.dbg & 4)) {              // diagnostics: every k tile re-reads the block's FIRST tile (L1 / L2 resident)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int i = 0; i < MT; ++i) { sa[q][i].step = 0; sa[q][i].sstep = 0; }
                sb[q].step = 0; sb[q].sstep = 0;
            }
        }
        const bool do_colsum = (BMODE == OP_XC) && g.colsum != nullptr && tm == 0;
        float csum = 0.0f;
#define BXW_FETCH(Q, T)                                                                                        \
        if ((T) < nfull) {                                                                                     \
            _Pragma("unroll") for (int i = 0; i < MT; ++i) sa[Q][i].fetch();                                   \
            sb[Q].fetch();                                                                                     \
        } else {                                                                                               \
            _Pragma("unroll") for (int i = 0; i < MT; ++i) sa[Q][i].fetch_partial(kb + (T) * 16, ke, lt);      \
            sb[Q].fetch_partial(kb + (T) * 16, ke, lt);                                                        \
        }
#define BXW_COMMIT(Q, ST)                                                                                      \
        if (do_colsum) csum += sb[Q].sum8();                                                                   \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) sa[Q][i].commit(smem + (ST) * STAGE);                   \
        sb[Q].commit(smem + (ST) * STAGE + A_OPER);
        // diagnostics (PROF instantiation only; results are wrong): g.dbg & 1 = no global loads inside the loop,
        // g.dbg & 2 = no split / LDS writes inside the loop
        const bool ld_on = !(PROF && (g.dbg & 1)), cm_on = !(PROF && (g.dbg & 2));
        if (nk > 0) {
            BXW_FETCH(0, 0)
            if (nk > 1) { BXW_FETCH(1, 1) }
            BXW_COMMIT(0, 0)
            if (nk > 2) { BXW_FETCH(0, 2) }
        }
        bx_barrier();
        if (PROF) { p_loop = plast = __builtin_amdgcn_s_memtime(); }
        // stamped instantiation: [2] = the wait for the tile about to be split (the loads of the tile after it are younger)
        constexpr int NLD = MT * (AMODE == OP_KC ? 2 : 8) + (BMODE == OP_KC ? 2 : 8);
        for (int kt = 0; kt < nk; kt += 2) {
            if (PROF && kt + 3 < nk && g.gather == nullptr) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLD) : "memory"); BX_STAMP(2) }
            if (kt + 1 < nk) {                      // tile kt + 1 sits in set 1
                if (cm_on) { BXW_COMMIT(1, 1) }
                if (kt + 3 < nk && ld_on) { BXW_FETCH(1, kt + 3) }
            }
            BX_STAMP(3)
            bx_barrier();
            BX_STAMP(4)
            if (kt + 1 >= nk) break;
            if (PROF && kt + 4 < nk && g.gather == nullptr) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NLD) : "memory"); BX_STAMP(2) }
            if (kt + 2 < nk) {                      // tile kt + 2 sits in set 0
                if (cm_on) { BXW_COMMIT(0, 0) }
                if (kt + 4 < nk && ld_on) { BXW_FETCH(0, kt + 4) }
            }
            BX_STAMP(3)
            bx_barrier();
            BX_STAMP(4)
        }
#undef BXW_FETCH
#undef BXW_COMMIT
        if (PROF) p_exit_loop = __builtin_amdgcn_s_memtime();
        if (do_colsum && lt >= 128) s_cs[lt - 128] = csum;
        bx_barrier();
        if (do_colsum && lt < 128 && n0 + lt < g.N) g.colsum[(long long)z * g.colsum_slab + n0 + lt] = csum + s_cs[lt];
    } else {
        // ---------------------------------------------------------------- multipliers
        const int wm = wave >> 1, wn = wave & 1;
        const int l31 = lane & 31, khalf = lane >> 5;
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        const int fa = khalf * (XA * 16) + (wm * 64 + l31) * 16, fb = khalf * 2048 + (wn * 64 + l31) * 16;
        bx_barrier();
        if (PROF) { p_loop = plast = __builtin_amdgcn_s_memtime(); }
        for (int kt = 0; kt < nk; ++kt) {
            const unsigned char* at = smem + (kt & 1) * STAGE;
            const unsigned char* bt = at + A_OPER;
            bf16x8_t a[3][2], b[3][2];
#pragma unroll
            for (int pl = 2; pl >= 0; --pl)            // the planes of the first terms first
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[pl][i] = *reinterpret_cast<const bf16x8_t*>(at + pl * A_PLANE + fa + i * 512);
                    b[2 - pl][i] = *reinterpret_cast<const bf16x8_t*>(bt + (2 - pl) * BX_PLANE + fb + i * 512);
                }
#define BX_TERM(PA, PB)                                                                                        \
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][0], b[PB][0], acc[0][0], 0, 0, 0);            \
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][0], b[PB][1], acc[0][1], 0, 0, 0);            \
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][1], b[PB][0], acc[1][0], 0, 0, 0);            \
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA][1], b[PB][1], acc[1][1], 0, 0, 0);
            BX_TERM(2, 0) BX_TERM(0, 2) BX_TERM(1, 1) BX_TERM(1, 0) BX_TERM(0, 1) BX_TERM(0, 0)
#undef BX_TERM
            BX_STAMP(2)
            bx_barrier();
            BX_STAMP(4)
        }
        if (PROF) p_exit_loop = __builtin_amdgcn_s_memtime();
        bx_barrier();
        store_tile<EM>(g, acc, reinterpret_cast<float*>(smem), z, m0, n0, tn, tilesN, wave, lane);
    }
    if (PROF && g.prof != nullptr && lane == 0) {
        __builtin_amdgcn_s_waitcnt(0);
        const unsigned long long p_end = __builtin_amdgcn_s_memtime();
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* o = g.prof + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (NMW + 4) + wave) * 8;
        o[0] = p_entry; o[1] = p_loop; o[2] = pacc[2]; o[3] = pacc[3]; o[4] = pacc[4]; o[5] = p_exit_loop; o[6] = p_end;
        o[7] = ((unsigned long long)xcc << 32) | hw;
    }
}

// ---- 256 x 256 block tile, eight waves of 128 x 64 (GemmArgs::bx3 == 3) -------------------------------------------------------
// Per MFMA this tile needs half of everything the 128 x 128 kernels need beside the matrix pipe: 32 KiB of operands, 16 values
// to split per thread and 18 fragment reads per 48 MFMAs of a wave (2.6 issued instructions per MFMA instead of 5.0, 10.7
// instead of 21 bytes per cycle and CU at the pipe's full rate).  One block per CU, two waves per SIMD -- waves w and w + 4 --
// and those two run the k tile in OPPOSITE order so that they do not both want the matrix pipe right behind the barrier:
// waves 0-3 read their fragments, multiply, then split and write their share of the next tile; waves 4-7 split and write
// first (their loads were issued a whole iteration earlier), then read and multiply.  Same LDS image per 128 rows / columns,
// k order and term order as k_gemm_bx3: the same bits for the same K split.
// Edge tiles (gemm_edge.h): a wave whose 128 x 64 sub-tile lies outside M x N -- rows 128 .. 255 of a last row tile of at most 128
// rows, the column slices behind N in the last column tile -- runs a k loop of staging and barriers only and leaves the matrix pipe
// of its SIMD to the wave beside it; where at most four sub-tiles are live they sit on waves 0-3, one per SIMD (a sliver of at most
// 128 columns beside full rows is the one extent the plain map would pair on SIMDs 0 / 1: remapped).  Which wave computes a
// sub-tile changes nothing in it; a dead wave's epilogue writes what it always wrote (nothing, or the empty softmax partials of
// its slices).  `wave` is what STAGING goes by (stager rows, LDS-DMA regions, the ep slice, late, column sums), (wm, wn) the sub-tile.
// QUEUE (GemmArgs::xcd_first != 0): the tile comes from the work queue of k_gemm_queue instead of blockIdx -- a restricted launch
// (xcd_first > 0) lets only blocks on XCDs >= xcd_first draw, only items below work_limit and only while *stop == 0; the clean-up
// launch (xcd_first < 0) takes what nobody claimed.  Which block computes an item never changes the item.
// AG: two-part op(A) (GemmArgs::m_split; x-contiguous operands through LDS-DMA only)
template <int AMODE, int BMODE, bool PROF = false, int BUFM = 0, bool QUEUE = false, bool AG = false, int EM = EPI_PLAIN>
__global__ __launch_bounds__(512, 1) void k_gemm_bx3h(const GemmArgs g) {
    constexpr int XT = 256;
    constexpr int PLANE = 2 * XT * 16, OPER = 3 * PLANE;                              // 8 KiB, 24 KiB
    constexpr int EPI = 8 * 32 * 68 * 4;
    constexpr bool DMA = BUFM >= 3;                       // x-contiguous operands through LDS-DMA (BxDmaXC)
    constexpr int A_BYTES = 2 * OPER, PIPE = 4 * OPER;    // two LDS stages per operand: 96 KiB
    static_assert(PIPE >= EPI, "the epilogue's transpose slices live in the pipeline's LDS");
    constexpr int RAW = DMA ? ((AMODE == OP_XC) + (BMODE == OP_XC)) * 8 * 2048 : 0;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[PIPE + RAW];
    __shared__ float s_cs[256];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool late = wave >= 4;                          // order of the k tile, see above
    const int l31 = lane & 31, khalf = lane >> 5;
    const int tilesM = (g.M + XT - 1) / XT, tilesN = (g.N + XT - 1) / XT;
    int tm, tn, z;
    if (QUEUE) {
        __shared__ int s_item;
        const int total = tilesM * tilesN * (g.ksplit > 1 ? g.ksplit : 1);
        if (g.xcd_first > 0) {
            int xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            // below xcd_first: the XCDs of the kernel this launch runs beside.  A block can only be placed there before that kernel
            // has taken its CUs (leave at once) or after it has left them (gated launches: join the drawing when it is really over)
            if ((xcc & 7) < g.xcd_first) {
                if (g.gate == nullptr) return;
                // ONE thread decides for the block: the counter may be completing while the block reads it, and a block whose threads
                // disagree would go on with half its waves (first version: half-computed tiles, one step in three)
                if (tid == 0) s_item = __hip_atomic_load(g.gate + g.gate_last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= g.gate_expect;
                __syncthreads();
                const int join = s_item;
                __syncthreads();
                if (!join) return;
            }
        }
        if (tid == 0) {
            int item = -1;
            if (g.xcd_first < 0) {
                const int j = atomicAdd(g.work + 1, 1);
                if (j < total && atomicCAS(g.claim + j, 0, 1) == 0) item = j;
            } else if (__hip_atomic_load(g.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
                const int j = atomicAdd(g.work, 1);
                if (j < min(g.work_limit, total) && atomicCAS(g.claim + j, 0, 1) == 0) item = j;
            }
            if (item >= 0 && g.gate != nullptr) {          // wait for the last time step the tile's rows belong to
                const int tm_ = (item / tilesN) % tilesM;
                int t_need = (min(g.M, (tm_ + 1) * XT) - 1) / g.gate_rows;
                if (g.gate_every > 1) t_need = min(g.gate_last, (t_need / g.gate_every + 1) * g.gate_every - 1);
                const int spin_cap = g.gate_spin;
                for (int spins = 0; __hip_atomic_load(g.gate + t_need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < g.gate_expect; ++spins) {
                    __builtin_amdgcn_s_sleep(32);
                    if (spins >= spin_cap || ((spins & 63) == 63 && __hip_atomic_load(g.gate_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 2)) {
                        __hip_atomic_store(g.gate_err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        item = -1;
                        break;
                    }
                }
            }
            s_item = item;
        }
        __syncthreads();
        const int item = s_item;
        if (item < 0) return;
        // The rows were written (write-through) by another XCD while this launch was running, and are read with ordinary loads:
        // this XCD's L2 was invalidated when the launch started (the acquire of every kernel dispatch -- what makes any producer /
        // consumer pair of kernels on different XCDs work), and a row enters it only through loads issued behind that row's gate.
        // Measured (profiles/r04_xov_*.log) and removed: an agent-scope acquire here emptied the L2 for every block of the XCD
        // (920 times in 0.5 ms; 105 instead of 85 us per tile), agent-scope (sc1) loads of the operand bypassed the L2 (the same 105 us).
        tm = (item / tilesN) % tilesM; tn = item % tilesN; z = item / (tilesM * tilesN);
    } else {
        const int bid = xcd_tile(blockIdx.x, tilesM * tilesN);
        tile_coords(bid, tilesM, tilesN, g.group_m, tm, tn);
        z = blockIdx.y;
    }
#include "gemm_bx3h_tile.h"
}

// Clean-up launch over the work lists of TWO x-contiguous x x-contiguous GEMMs (GemmPairArgs): joint items [0, n0) are g0's -- what the
// restricted launch of g0 ALONE (k_gemm_bx3h<..., QUEUE>, the same work / claim words) has not claimed --, [n0, n0 + n1) are g1's, a
// two-part-A GEMM nobody else draws from.  One draw per block, as in the clean-up launch of one GEMM; the item then runs the statements
// (gemm_bx3h_tile.h) of the instantiation its GEMM takes alone -- g0: <OP_XC, OP_XC, BUFM = 3>, g1: the same with AG --, so which launch
// computes an item never changes the item.  A uniform branch, not AG as a run-time value: each side keeps its own stager type.
// g0.gate_err (optional): 2 there -- the kernel that produced the operands gave up, the step is skipped -- and the block leaves before drawing.
__global__ __launch_bounds__(512, 1) void k_gemm_bx3h_pair(const GemmPairArgs p) {
    constexpr int AMODE = OP_XC, BMODE = OP_XC, BUFM = 3, EM = EPI_PLAIN;
    constexpr bool PROF = false;
    constexpr int XT = 256;
    constexpr int PLANE = 2 * XT * 16, OPER = 3 * PLANE;
    constexpr bool DMA = BUFM >= 3;
    constexpr int A_BYTES = 2 * OPER, PIPE = 4 * OPER;
    constexpr int RAW = 2 * 8 * 2048;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[PIPE + RAW];
    __shared__ float s_cs[256];
    __shared__ int s_item;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool late = wave >= 4;
    const int l31 = lane & 31, khalf = lane >> 5;
    if (tid == 0) {
        int item = -1;
        if (p.g0.gate_err == nullptr || __hip_atomic_load(p.g0.gate_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 2) {
            // g1's items are drawn FIRST.  A launch's blocks are dealt to the XCDs in turn and an XCD that is free runs through its share at
            // once: with g0's (mostly claimed) items in front, the XCDs the chain has just left used up the draws that end in an exit and
            // g1's 240 items at cfg-B fell to the 160 CUs of the others -- two rounds (measured: 274 us against 21 + 102 us for the two launches)
            const int j = atomicAdd(p.g0.work + 1, 1);
            const int it = j < p.n1 ? p.n0 + j : j - p.n1;
            if (j < p.n0 + p.n1 && atomicCAS(p.g0.claim + it, 0, 1) == 0) item = it;
        }
        s_item = item;
    }
    __syncthreads();
    const int item = __builtin_amdgcn_readfirstlane(s_item);
    if (item < 0) return;
    if (item < p.n0) {
        constexpr bool AG = false;
        const GemmArgs& g = p.g0;
        const int tilesM = (g.M + XT - 1) / XT, tilesN = (g.N + XT - 1) / XT;
        const int tm = (item / tilesN) % tilesM, tn = item % tilesN, z = item / (tilesM * tilesN);
#include "gemm_bx3h_tile.h"
    } else {
        constexpr bool AG = true;
        const GemmArgs& g = p.g1;
        const int it = item - p.n0;
        const int tilesM = (g.M + XT - 1) / XT, tilesN = (g.N + XT - 1) / XT;
        const int tm = (it / tilesN) % tilesM, tn = it % tilesN, z = it / (tilesM * tilesN);
#include "gemm_bx3h_tile.h"
    }
}
#undef BX_STAMP

// Launch of a bf16-split kernel with the epilogue's mode as its last template argument.  The two cross-entropy modes exist for the
// projection's operand layout only (A k-contiguous, B x-contiguous: launch_t refuses them elsewhere), so only that layout carries
// three instantiations per kernel form.
#define FSMG_LAUNCH_EPI(GRID, BLOCK, LDS, KERNEL, ...)                                                                          \
    do {                                                                                                                        \
        if constexpr (AMODE == OP_KC && BMODE == OP_XC) {                                                                       \
            if (em == EPI_CE_STORE) { hipLaunchKernelGGL((KERNEL<__VA_ARGS__, EPI_CE_STORE>), GRID, BLOCK, LDS, s, g); break; } \
            if (em == EPI_CE_FWD) { hipLaunchKernelGGL((KERNEL<__VA_ARGS__, EPI_CE_FWD>), GRID, BLOCK, LDS, s, g); break; }     \
        }                                                                                                                       \
        hipLaunchKernelGGL((KERNEL<__VA_ARGS__, EPI_PLAIN>), GRID, BLOCK, LDS, s, g);                                           \
    } while (0)

template <int AMODE, int BMODE>
hipError_t launch_t(hipStream_t s, const GemmArgs& g, int lds_pad) {
    const int tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN;
    // weighted column sums: the 256 x 256-tile kernels' x-contiguous-operand instantiations only; exp(logit) stores: the bf16-split kernels
    if (g.colsum_w != nullptr && !(g.bx3 == 3 && AMODE == OP_XC && BMODE == OP_XC && g.colsum != nullptr)) return hipErrorInvalidValue;
    if (g.ce_store && !(g.bx3 != 0 && g.ce_part != nullptr && g.ksplit <= 1)) return hipErrorInvalidValue;      // (every bf16-split kernel: one epilogue)
    // the epilogue's mode, a template argument of the bf16-split kernels (store_tile_at).  Where one of them will really run -- bx3 != 0,
    // and for a work-queue launch bx3 == 3: the others take the fp32-MFMA k_gemm_queue, whose mode stays a run-time property -- the two
    // cross-entropy modes exist for the projection's operand layout only (GemmArgs::ce_part)
    const int em = g.ce_part == nullptr ? EPI_PLAIN : g.ce_store ? EPI_CE_STORE : EPI_CE_FWD;
    const bool split_kernel = g.bx3 != 0 && (g.xcd_first == 0 || g.bx3 == 3);
    if (split_kernel && em != EPI_PLAIN && !(AMODE == OP_KC && BMODE == OP_XC)) return hipErrorInvalidValue;
    if (g.xcd_first != 0 && g.bx3 == 3) {      // work-queue launch of the 256 x 256-tile kernel (one block per CU)
        if (g.work == nullptr || g.claim == nullptr || (g.xcd_first > 0 && g.stop == nullptr) || g.gather != nullptr || g.prof != nullptr) return hipErrorInvalidValue;
        const long long a_b = 4LL * g.lda * (AMODE == OP_KC ? g.M : g.K), b_b = 4LL * g.ldb * (BMODE == OP_KC ? g.N : g.K);
        if (a_b >= 0xfffff000LL || b_b >= 0xfffff000LL) return hipErrorInvalidValue;
        const int total = ((g.M + 255) / 256) * ((g.N + 255) / 256) * (g.ksplit > 1 ? g.ksplit : 1);
        const int lim = g.work_limit < total ? g.work_limit : total;
        const int blocks = g.xcd_first > 0 ? (int)(((long long)lim * 8 + 7 - g.xcd_first) / (8 - g.xcd_first)) + 64 : total;
        const bool a_dma = AMODE != OP_XC || (g.lda % 4 == 0 && g.M % 4 == 0 && ((uintptr_t)g.A & 15) == 0);
        const bool b_dma = BMODE != OP_XC || (g.ldb % 4 == 0 && g.N % 4 == 0 && ((uintptr_t)g.B & 15) == 0);
        if constexpr (AMODE == OP_XC && BMODE == OP_XC) {
            if (g.m_split > 0) {       // two-part op(A) from the queue (round 6: dKx + dKh of the layer above beside a BPTT chain)
                const bool ok = g.m_split % 256 == 0 && g.m_split < g.M && g.A2 != nullptr && b_dma && g.lda % 4 == 0 && g.lda2 % 4 == 0 &&
                                (g.M - g.m_split) % 4 == 0 && (((uintptr_t)g.A | (uintptr_t)g.A2) & 15) == 0 && 4LL * g.lda2 * g.K < 0xfffff000LL;
                if (!ok) return hipErrorInvalidValue;
                FSMG_LAUNCH_EPI(dim3(blocks), dim3(512), 0, k_gemm_bx3h, AMODE, BMODE, false, 3, true, true);
                return hipGetLastError();
            }
            if (a_dma && b_dma) { FSMG_LAUNCH_EPI(dim3(blocks), dim3(512), 0, k_gemm_bx3h, AMODE, BMODE, false, 3, true, false); return hipGetLastError(); }
        }
        if (g.m_split > 0) return hipErrorInvalidValue;
        FSMG_LAUNCH_EPI(dim3(blocks), dim3(512), 0, k_gemm_bx3h, AMODE, BMODE, false, 2, true, false);
        return hipGetLastError();
    }
    if (g.xcd_first != 0) {             // work-queue launch: one resident set of blocks (4 per CU), see k_gemm_queue
        if (g.work == nullptr || g.claim == nullptr || (g.xcd_first > 0 && g.stop == nullptr) || (AMODE == OP_XC && g.gather != nullptr)) return hipErrorInvalidValue;
        const int total = tilesM * tilesN * (g.ksplit > 1 ? g.ksplit : 1);
        // a restricted launch needs as many blocks on the XCDs that may draw as there are items below its limit
        const int lim = g.work_limit < total ? g.work_limit : total;
        const int blocks = g.xcd_first > 0 ? (int)(((long long)lim * 8 + 7 - g.xcd_first) / (8 - g.xcd_first)) + 64 : total;
        hipLaunchKernelGGL((k_gemm_queue<AMODE, BMODE>), dim3(blocks), dim3(NTHREADS), lds_pad, s, g);
        return hipGetLastError();
    }
    dim3 grid(tilesM * tilesN, g.ksplit > 1 ? g.ksplit : 1);
    // buffer loads (32-bit offsets) for the operands that fit 4 GiB and whose rows are not gathered along K; a gathered KC
    // operand (embedding rows by token id) keeps 64-bit addresses too: its extent is the table's, which this call does not know
    const long long a_bytes = 4LL * g.lda * (AMODE == OP_KC ? g.M : g.K), b_bytes = 4LL * g.ldb * (BMODE == OP_KC ? g.N : g.K);
    const bool a_buf = g.gather == nullptr && a_bytes < 0xfffff000LL, b_buf = b_bytes < 0xfffff000LL;
    static const bool buf_off = std::getenv("FSMG_GEMM_BUF") && std::atoi(std::getenv("FSMG_GEMM_BUF")) == 0;      // A/B runs
    const int bufm = (buf_off && g.prof == nullptr) ? 0 : (a_buf && b_buf) ? 2 : (b_buf ? 1 : 0);
#ifdef FSMG_EXPERIMENTS
    if (g.prof != nullptr && bufm != 2) return hipErrorInvalidValue;     // the stamped instantiations exist for bufm == 2 only
#else
    if (g.prof != nullptr) return hipErrorInvalidValue;                  // stamped instantiations + ablations: experiment builds only (make experiments)
#endif
    if (g.bx3 == 3) {        // 256 x 256 tile
        dim3 grid3(((g.M + 255) / 256) * ((g.N + 255) / 256), g.ksplit > 1 ? g.ksplit : 1);
        if (g.m_split > 0) {    // two-part op(A): [gathered or plain | plain], both parts and B through LDS-DMA
            if constexpr (AMODE == OP_XC && BMODE == OP_XC) {
                const bool ok = g.m_split % 256 == 0 && g.m_split < g.M && g.A2 != nullptr && g.prof == nullptr && b_buf &&
                                g.lda % 4 == 0 && g.lda2 % 4 == 0 && (g.M - g.m_split) % 4 == 0 && g.ldb % 4 == 0 && g.N % 4 == 0 &&
                                (((uintptr_t)g.A | (uintptr_t)g.A2 | (uintptr_t)g.B) & 15) == 0 && 4LL * g.lda2 * g.K < 0xfffff000LL &&
                                (g.gather != nullptr || 4LL * g.lda * g.K < 0xfffff000LL);
                if (!ok) return hipErrorInvalidValue;
                FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, false, 3, false, true);
                return hipGetLastError();
            }
            return hipErrorInvalidValue;
        }
        // x-contiguous operands through LDS-DMA where their shape allows 16-byte row pieces (BxDmaXC)
        const bool dma_off = !gemm_dma_enabled();
        const bool a_dma = AMODE != OP_XC || (g.lda % 4 == 0 && g.M % 4 == 0 && ((uintptr_t)g.A & 15) == 0);
        const bool b_dma = BMODE != OP_XC || (g.ldb % 4 == 0 && g.N % 4 == 0 && ((uintptr_t)g.B & 15) == 0);
        // (measured: 4760 -> 3880 cycles per k tile with two x-contiguous operands, 16 -> 4 loads per thread and tile; with one,
        // 10 -> 4 loads, 3700 -> 3820: not used there)
        const bool dma = !dma_off && bufm == 2 && a_dma && b_dma;
        if constexpr (AMODE == OP_XC && BMODE == OP_XC) {
#ifdef FSMG_EXPERIMENTS
            if (dma && g.prof != nullptr) { FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, true, 3, false, false); return hipGetLastError(); }
#endif
            if (dma) { FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, false, 3, false, false); return hipGetLastError(); }
        }
#ifdef FSMG_EXPERIMENTS
        if (g.prof != nullptr) { FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, true, 2, false, false); return hipGetLastError(); }
#endif
        if (bufm == 2) FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, false, 2, false, false);
        else if (bufm == 1) FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, false, 1, false, false);
        else FSMG_LAUNCH_EPI(grid3, dim3(512), lds_pad, k_gemm_bx3h, AMODE, BMODE, false, 0, false, false);
        return hipGetLastError();
    }
    if (g.bx3 == 2) {        // wave-specialised variant
#ifdef FSMG_EXPERIMENTS
        if (g.prof != nullptr) { FSMG_LAUNCH_EPI(grid, dim3(512), lds_pad, k_gemm_bx3w, AMODE, BMODE, 1, true, 2); return hipGetLastError(); }
#endif
        if (bufm == 2) FSMG_LAUNCH_EPI(grid, dim3(512), lds_pad, k_gemm_bx3w, AMODE, BMODE, 1, false, 2);
        else if (bufm == 1) FSMG_LAUNCH_EPI(grid, dim3(512), lds_pad, k_gemm_bx3w, AMODE, BMODE, 1, false, 1);
        else FSMG_LAUNCH_EPI(grid, dim3(512), lds_pad, k_gemm_bx3w, AMODE, BMODE, 1, false, 0);
        return hipGetLastError();
    }
    if (g.bx3) {             // (gathered K rows included: BxStager)
#ifdef FSMG_EXPERIMENTS
        if (g.prof != nullptr) { FSMG_LAUNCH_EPI(grid, dim3(256), lds_pad, k_gemm_bx3, AMODE, BMODE, true, 2); return hipGetLastError(); }
#endif
        if (bufm == 2) FSMG_LAUNCH_EPI(grid, dim3(256), lds_pad, k_gemm_bx3, AMODE, BMODE, false, 2);
        else if (bufm == 1) FSMG_LAUNCH_EPI(grid, dim3(256), lds_pad, k_gemm_bx3, AMODE, BMODE, false, 1);
        else FSMG_LAUNCH_EPI(grid, dim3(256), lds_pad, k_gemm_bx3, AMODE, BMODE, false, 0);
        return hipGetLastError();
    }
    // lds_pad: unused dynamic LDS that only lowers the number of co-resident blocks per CU
    // rows of a gathered XC operand change with k: that one (dKx) keeps the register-staged kernel
    if (AMODE == OP_XC && g.gather != nullptr) hipLaunchKernelGGL((k_gemm_staged<OP_XC, OP_XC>), grid, dim3(NTHREADS), lds_pad, s, g);
    else hipLaunchKernelGGL((k_gemm<AMODE, BMODE>), grid, dim3(NTHREADS), lds_pad, s, g);
    return hipGetLastError();
}
#undef FSMG_LAUNCH_EPI

__global__ void k_reduce_slabs(const float* __restrict__ slabs, long long stride, int nslab,
                               float* __restrict__ out, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += step) {
        float s = slabs[i];
        for (int z = 1; z < nslab; ++z) s += slabs[z * stride + i];
        out[i] = s;
    }
}

// blocks [0, nb1): range 1, the rest: range 2 -- the same per-element sum as k_reduce_slabs
__global__ void k_reduce_slabs2(const float* __restrict__ slabs, long long stride, int nslab, float* __restrict__ out, long long n,
                                int nb1, const float* __restrict__ slabs2, long long stride2, float* __restrict__ out2, long long n2) {
    const bool second = (int)blockIdx.x >= nb1;
    const float* sl = second ? slabs2 : slabs;
    float* o = second ? out2 : out;
    const long long st = second ? stride2 : stride, nn = second ? n2 : n;
    const long long b = second ? (long long)blockIdx.x - nb1 : blockIdx.x, nb = second ? (long long)gridDim.x - nb1 : nb1;
    for (long long i = b * blockDim.x + threadIdx.x; i < nn; i += nb * blockDim.x) {
        float v = sl[i];
        for (int z = 1; z < nslab; ++z) v += sl[z * st + i];
        o[i] = v;
    }
}

}  // namespace

int gemm_block_slots() { return 256 * ((BK == 16 ? 4 : 2) * 256 / NTHREADS); }
int gemm_tile_m() { return BM; }
bool gemm_dma_enabled() {
    static const bool off = std::getenv("FSMG_GEMM_DMA") && std::atoi(std::getenv("FSMG_GEMM_DMA")) == 0;
    return !off;
}
// dynamic-LDS padding that caps the resident blocks per CU (160 KiB LDS) when a GEMM runs beside the recurrent-step
// kernels on the auxiliary stream.  The padded block is just too big for blocks_per_cu + 1 of them to fit, NOT
// 1/blocks_per_cu of the LDS: the first version of this cap handed the GEMM blocks all 160 KiB, so a step-kernel
// block (4-9 KiB of LDS) could only be placed on a CU when a GEMM block retired, and a step co-running with the dW
// GEMM took 15.8 us instead of 6.4.  With this sizing the capped blocks leave >= 36 KiB per CU.
int gemm_lds_pad_for(int blocks_per_cu) {
    constexpr int own = 4 * 32 * 68 * 4;                            // static LDS of one block (epilogue > pipeline)
    const int max_blocks = (BK == 16 ? 4 : 2) * 256 / NTHREADS;
    if (blocks_per_cu >= max_blocks) return 0;
    const int block = (160 * 1024) / (blocks_per_cu + 1) + 1024;    // blocks_per_cu + 1 of these exceed 160 KiB
    return block > own ? block - own : 0;
}

hipError_t launch_gemm(hipStream_t s, int amode, int bmode, const GemmArgs& g, int lds_pad) {
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    if (amode == OP_KC && bmode == OP_XC) return launch_t<OP_KC, OP_XC>(s, g, lds_pad);
    if (amode == OP_XC && bmode == OP_XC) return launch_t<OP_XC, OP_XC>(s, g, lds_pad);
    if (amode == OP_KC && bmode == OP_KC) return launch_t<OP_KC, OP_KC>(s, g, lds_pad);
    return hipErrorInvalidValue;
}

static int pair_items(const GemmArgs& g) { return ((g.M + 255) / 256) * ((g.N + 255) / 256) * (g.ksplit > 1 ? g.ksplit : 1); }
// what launch_t asks of a work-queue launch of either GEMM alone before it takes the LDS-DMA staged instantiations: the joint launch runs those
bool gemm_pair_supported(const GemmArgs& g0, const GemmArgs& g1) {
    auto plain = [](const GemmArgs& g) {
        return g.M > 0 && g.N > 0 && g.ce_part == nullptr && g.prof == nullptr && g.gate == nullptr &&
               g.ldb % 4 == 0 && g.N % 4 == 0 && ((uintptr_t)g.B & 15) == 0 && 4LL * g.ldb * g.K < 0xfffff000LL;
    };
    if (!plain(g0) || !plain(g1)) return false;
    if (g0.m_split != 0 || g0.gather != nullptr || g0.lda % 4 != 0 || g0.M % 4 != 0 || ((uintptr_t)g0.A & 15) != 0 || 4LL * g0.lda * g0.K >= 0xfffff000LL) return false;
    return g1.m_split > 0 && g1.m_split % 256 == 0 && g1.m_split < g1.M && g1.A2 != nullptr && g1.lda % 4 == 0 && g1.lda2 % 4 == 0 &&
           (g1.M - g1.m_split) % 4 == 0 && (((uintptr_t)g1.A | (uintptr_t)g1.A2) & 15) == 0 && 4LL * g1.lda2 * g1.K < 0xfffff000LL &&
           (g1.gather != nullptr || 4LL * g1.lda * g1.K < 0xfffff000LL);
}
hipError_t launch_gemm_pair_cleanup(hipStream_t s, const GemmArgs& g0, const GemmArgs& g1) {
    if (!gemm_pair_supported(g0, g1) || g0.work == nullptr || g0.claim == nullptr || g0.bx3 != 3 || g1.bx3 != 3) return hipErrorInvalidValue;
    GemmPairArgs p{};
    p.g0 = g0; p.g1 = g1; p.n0 = pair_items(g0); p.n1 = pair_items(g1);
    p.g0.xcd_first = p.g1.xcd_first = -1;
    hipLaunchKernelGGL(k_gemm_bx3h_pair, dim3(p.n0 + p.n1), dim3(512), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_reduce_slabs2(hipStream_t s, const float* slabs, long long slab_stride, int nslab, float* out, long long n,
                                const float* slabs2, long long slab_stride2, float* out2, long long n2) {
    if (n2 <= 0) return launch_reduce_slabs(s, slabs, slab_stride, nslab, out, n);
    if (n <= 0) return launch_reduce_slabs(s, slabs2, slab_stride2, nslab, out2, n2);
    int nb1 = (int)std::min<long long>((n + 255) / 256, 2048), nb2 = (int)std::min<long long>((n2 + 255) / 256, 64);
    hipLaunchKernelGGL(k_reduce_slabs2, dim3(nb1 + nb2), dim3(256), 0, s, slabs, slab_stride, nslab, out, n, nb1, slabs2, slab_stride2, out2, n2);
    return hipGetLastError();
}

hipError_t launch_reduce_slabs(hipStream_t s, const float* slabs, long long slab_stride, int nslab,
                               float* out, long long n) {
    if (n <= 0) return hipSuccess;
    int blocks = (int)((n + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(k_reduce_slabs, dim3(blocks), dim3(256), 0, s, slabs, slab_stride, nslab, out, n);
    return hipGetLastError();
}

}  // namespace fsmg
