// Internal launcher interface between the C-ABI orchestration (api_*.hip behind fsmg_model.h) and the
// gfx950 kernels.  Nothing here is exported; include/fsmg.h is the public surface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsmg {

// ---------------------------------------------------------------- GEMM (gemm.hip)
// C[M,N] (+)= op(A)[M,K] * op(B)[K,N], fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32.
// Operand storage modes (what is contiguous in HBM):
//   KC: the K index is contiguous  (A stored [M][K] / B stored [N][K])
//   XC: the non-K index is contiguous (A stored [K][M] / B stored [K][N])
enum { OP_KC = 0, OP_XC = 1 };
struct GemmArgs {
    const float* A; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    int M, N, K;
    const float* bias;      // optional [N], added in the epilogue
    const int* gather;      // optional row gather for A: KC -> M-rows, XC -> K-rows index into A
    float* colsum;          // optional [N]: column sums of op(B) over K (XC B only), written by M-tile 0
    int ksplit;             // >= 1; slab z covers a K range, C/colsum slab stride below
    long long c_slab;       // elements between consecutive K-split slabs of C
    long long colsum_slab;
    // forward-only cross entropy: when ce_part != nullptr C is NOT stored; instead every wave writes, per row of its
    // 64-column slice, (max, sum exp(x - max)) over the columns < ce_nvocab into ce_part[row][2*tile_n + half] and
    // the logit of the row's target column into ce_tgt_logit[row]
    // On the bf16-split kernels (bx3 != 0) the cross-entropy epilogues -- this one and ce_store below -- are instantiated for the
    // projection's operand layout only, (OP_KC, OP_XC): launch_gemm returns hipErrorInvalidValue for the other two layouts there.
    float2* ce_part; const int* ce_tgt; float* ce_tgt_logit; int ce_nvocab;
    // ce_store != 0 (train passes, "fused softmax"): besides the partials the epilogue stores E = exp(x) (x = logit incl. bias; 0 in the
    // pad columns) into C -- the un-normalised softmax with NO shift, which launch_ce_finish turns into the loss gradient by patching
    // one element per row and handing a per-row scale to the two GEMMs that consume it.  The partial of a slice is (0, sum of its E):
    // no row maximum, no target lookup (launch_ce_finish takes the target logit as log(E[target])).  Valid while every row's sum and
    // target element stay normal fp32 numbers (CE_SUM_MIN / CE_SUM_MAX / CE_TGT_MIN: launch_ce_finish checks, the caller falls back
    // to launch_ce_rows otherwise).
    int ce_store;
    // column sums of op(B) weighted per K row (XC B, 256 x 256-tile kernel only): colsum[n] = sum_k colsum_w[k] * B[k][n]
    // (dd = sum_r c_r E'[r][v] of the fused softmax); colsum_w must be readable up to K rounded up to 16
    const float* colsum_w;
    // host-side plumbing (api_schedule.hip gemm()): C[m][:] is multiplied by row_scale[m] once it is complete -- in the deferred
    // slab sum where there is one, by launch_scale_rows otherwise.  The kernels ignore it.
    const float* row_scale;
    int nt_store;           // 1: C is written with non-temporal stores (streaming, read back much later)
    // Work-queue launches for the XCD-partitioned schedule (k_gemm_queue; not with `gather` on an XC operand).  Every block
    // draws one (split, row tile, column tile) item, row tiles slowest, in the order blocks start.  work[0] / work[1]: draw
    // counters of the restricted / clean-up launch, claim[items]: taken marks; all zeroed by the caller.
    //   xcd_first > 0: restricted launch -- only blocks on XCDs >= xcd_first draw, only items < work_limit, and only while
    //                  *stop == 0 (the caller raises it when the kernel that owned the other XCDs is done);
    //   xcd_first < 0: clean-up launch -- one block per item, computes the items nobody took.  Order it after everything
    //                  the remaining items read.
    // Placement decides speed, never results: an item is computed once, by the same code either way.
    int xcd_first; int* work; int* claim; int work_limit; const int* stop;
    // Gate of a work-queue launch whose A rows are still being produced by a kernel on the other XCDs (the overlapped step: the
    // projection beside the forward recurrence).  gate[t] reaches gate_expect when the rows of time step t (gate_rows rows each,
    // time-major) are in memory; a block that has drawn a row tile waits for the tile's last step, then takes an agent-scope
    // acquire.  Bounded: after gate_spin polls, or when *gate_err == 2 (the producer gave up), the block raises *gate_err = 2 and
    // leaves its tile uncomputed -- the step is skipped like any timed-out step.  Blocks of a restricted launch that land below
    // xcd_first join the drawing once gate[gate_last] is complete (the producer has left those XCDs).
    const int* gate; int gate_expect; int gate_rows; int gate_last; int* gate_err; int gate_spin;
    int gate_every;         // the producer publishes every gate_every-th step only (LstmFwdXcdArgs::progress_every): wait for the group's last
    int bx3;                // 1: k_gemm_bx3 -- fp32 product from three bf16 planes per operand on the bf16 matrix pipe (gemm.hip);
                            // 2: k_gemm_bx3w, its wave-specialised variant (same bits; two 512-thread blocks per CU)
    int group_m;                // bf16-split kernels: tile order, see tile_coords (gemm.hip); 0 = row tiles fastest
    unsigned long long* prof;   // diagnostics (tools/gemm_bench PROF=1, bx3 only): [blocks][waves][8] stamps, see k_gemm_bx3
    int dbg;                    // diagnostics, stamped instantiations only: ablation bits (k_gemm_bx3w: 1, 2, 4; k_gemm_bx3h: 8), results are wrong
    // Two-part op(A) of an XC x XC product on the 256 x 256-tile kernel (the merged weight gradient [x | h_prev]^T dZ of a layer: one
    // launch, one K split, one set of slabs for what were two GEMMs over the same dZ).  m_split > 0: rows [0, m_split) of op(A) are
    // the columns of A -- K rows gathered through `gather` when it is set (the caller guarantees the gathered table < 4 GiB) --,
    // rows [m_split, M) the columns of A2 (never gathered).  m_split is a multiple of 256.
    const float* A2; int lda2; int m_split;
};
// amode/bmode in {OP_KC, OP_XC}. Supported combinations: (KC,XC) (XC,XC) (KC,KC)
hipError_t launch_gemm(hipStream_t s, int amode, int bmode, const GemmArgs& g, int lds_pad = 0);
// The clean-up launch of a work-queue GEMM g0 (XC x XC, 256 x 256 tiles, LDS-DMA staged) with the items of a second one, g1 (the same with a
// two-part A, GemmArgs::m_split), as the tail of its list: joint item j < n0 is item j of g0, j >= n0 item j - n0 of g1.  g0.work[1] is the
// draw counter, g0.claim[0 .. n0 + n1) the taken marks (zeroed by the caller; the restricted launch of g0 ALONE marks what it took in
// [0, n0) and cannot draw from g1).  Blocks draw g1's items first, then what is left of g0's (k_gemm_bx3h_pair says why).  Ordered behind
// everything either GEMM reads; g1's queue words are not used.
// g0.gate_err != nullptr: a block that finds 2 there leaves before it draws.
struct GemmPairArgs { GemmArgs g0, g1; int n0, n1; };
bool gemm_pair_supported(const GemmArgs& g0, const GemmArgs& g1);
hipError_t launch_gemm_pair_cleanup(hipStream_t s, const GemmArgs& g0, const GemmArgs& g1);
// dynamic-LDS padding that caps a GEMM at `blocks_per_cu` resident blocks per CU
int gemm_lds_pad_for(int blocks_per_cu);
// resident 128x128 blocks the chip holds at once (256 CUs x blocks per CU): the split-K policy's slot count
int gemm_block_slots();
int gemm_tile_m();   // rows of a block tile (128 or 256)
bool gemm_dma_enabled();   // the 256-tile kernel stages x-contiguous operands through LDS-DMA (FSMG_GEMM_DMA=0: registers; A/B runs)
// out[i] = sum_z slabs[z][i]  (fixed order -> deterministic split-K)
hipError_t launch_reduce_slabs(hipStream_t s, const float* slabs, long long slab_stride, int nslab,
                               float* out, long long n);
// two such sums in one launch (a split-K GEMM's C and its column sums); the second may be empty (n2 == 0)
hipError_t launch_reduce_slabs2(hipStream_t s, const float* slabs, long long slab_stride, int nslab, float* out, long long n,
                                const float* slabs2, long long slab_stride2, float* out2, long long n2);

// ---------------------------------------------------------------- recurrent steps (lstm_step.hip)
struct LstmFwdArgs {
    const float* KhF;     // fragment-ordered recurrent weights (forward copy, see k_repack_kh)
    const float* hF_prev; // fragment-ordered h_{t-1}: [ceil(B/16)][Hp/16][64 lanes][4]
    float* hF_next;       // fragment-ordered h_t (written for step t+1)
    float* z;            // [B][4Hp] in: x-part pre-activations (+bias); out: activated gates i,j,f,o
    const float* c_prev; // [B][Hp]
    float* c_next;       // [B][Hp]
    float* h_next;       // [B][Hp]
    int B, Hp;
};
// prof != nullptr selects the instrumented build: per wave 8 s_memtime stamps (entry, loads landed,
// partials in LDS, past the barrier, done)
hipError_t launch_lstm_fwd_step(hipStream_t s, const LstmFwdArgs& a, unsigned long long* prof = nullptr);

// Persistent variant of the forward steps: ONE launch runs the time steps [t0, t1) of a layer.  Block (column tile,
// row tile) keeps its slice of the recurrent weights in registers for the whole launch; the blocks of a row tile
// hand h_t to each other through the fragment-ordered copy HF, whose time indices t0+1 .. t1 must be pre-filled
// with 0xFF bytes ("not written yet", see lstm_step.hip).  All blocks must be co-resident: check
// lstm_fwd_chain_supported() first.  A spin that does not complete sets *err_flag = 2 and every block leaves.
struct LstmFwdChainArgs {
    const float* KhF;     // forward fragment-ordered recurrent weights of the layer
    float* HF;            // [T+1][ceil(B/16)*16][Hp] fragment-ordered h, time index 0 = initial state
    float* Z;             // [T][B][4Hp] in: x-part pre-activations (+bias); out: activated gates
    float* Cs;            // [T+1][B][Hp]
    float* Hs;            // [T+1][B][Hp]
    int* err_flag;
    int B, Hp, T, t0, t1;
    int spin_limit;       // polls before a wave gives up (each ~0.5 us); 0 forces the timeout path (tests)
};
bool lstm_fwd_chain_supported(int B, int Hp);
hipError_t launch_lstm_fwd_chain(hipStream_t s, const LstmFwdChainArgs& a);
// Variant for shapes whose (column tile x row tile) grid does not fit the chip (H = 1024; 100-row episodes): a block
// owns a column tile for ALL row tiles (2..8) and walks them inside a step with the same resident weights.
bool lstm_fwd_chain_rt_supported(int B, int Hp);
hipError_t launch_lstm_fwd_chain_rt(hipStream_t s, const LstmFwdChainArgs& a);

struct LstmBwdArgs {
    const float* KhF;      // fragment-ordered recurrent weights (backward copy)
    const float* dzF_next; // fragment-ordered dz of step t+1: [ceil(B/16)][4Hp/16][64][4] (nullptr at the last step)
    float* dzF_cur;        // fragment-ordered dz of step t (written for step t-1)
    float* gates;         // [B][4Hp] in: activated gates of step t; out: dz of step t
    const float* c_t;     // [B][Hp]
    const float* c_prev;  // [B][Hp]
    float* dc;            // [B][Hp] carried cell gradient (in/out)
    const float* dh_top;  // [B][Hp] gradient arriving from above at step t
    int B, Hp;
};
hipError_t launch_lstm_bwd_step(hipStream_t s, const LstmBwdArgs& a, unsigned long long* prof = nullptr);

// Persistent variant of the backward steps: ONE launch runs BPTT for the time steps t1-1 down to t0 of a layer.  Same
// hand-off protocol as LstmFwdChainArgs; dz_t is handed over through dzF_all[t], whose indices t0 .. t1-1 must be
// pre-filled with 0xFF bytes.  Step t reads dzF_all[t+1] (skipped when t+1 == T: no recurrent gradient arrives).
struct LstmBwdChainArgs {
    const float* KhF;      // backward fragment-ordered recurrent weights of the layer
    float* dzF_all;        // [T][ceil(B/16)*16][4Hp] fragment-ordered dz per time step
    float* Z;              // [T][B][4Hp] in: activated gates; out: dz (row-major, for the weight-gradient GEMMs)
    const float* Cs;       // [T+1][B][Hp]
    float* dc;             // [B][Hp] carried cell gradient: read at t1-1, written back after t0
    const float* dH;       // [T][B][Hp] gradient arriving from above
    int* err_flag;
    int B, Hp, T, t0, t1;
    int spin_limit;
};
bool lstm_bwd_chain_supported(int B, int Hp);
hipError_t launch_lstm_bwd_chain(hipStream_t s, const LstmBwdChainArgs& a);

// Reduce-scatter form of the persistent backward steps.  Block j of a row tile owns 16 hidden units = 64 packed gate
// columns and keeps dz_t for those columns to itself; what travels is dh: after step t+1 it multiplies its dz slice
// with its COLUMN slice of Kh (all Hp units x 64 columns, resident in registers) and sends every block i the 16x16
// partial of dh_t that belongs to i's units (1 KiB), so a block receives Hp/16 KiB per step instead of the
// 16 x 4Hp x 4 B of dz the all-gather form reads.  inbox: [2 slots][row tiles][consumer][producer][64 lanes][4],
// every word 0xFFFFFFFF before the first launch of a pass (readers put the pattern back after reading).
struct LstmBwdRsArgs {
    const float* KhF;      // backward fragment-ordered recurrent weights of the layer
    float* inbox;
    float* Z;              // [T][B][4Hp] in: activated gates; out: dz (row-major, for the weight-gradient GEMMs)
    const float* Cs;       // [T+1][B][Hp]
    float* dc;             // [B][Hp] carried cell gradient: read at t1-1, written back after t0
    const float* dH;       // [T][B][Hp] gradient arriving from above
    int* err_flag;
    int B, Hp, T, t0, t1;
    int spin_limit;
};
bool lstm_bwd_rs_supported(int B, int Hp);
long long lstm_bwd_rs_inbox_floats(int B, int Hp);
hipError_t launch_lstm_bwd_rs(hipStream_t s, const LstmBwdRsArgs& a);
// recurrent weights [Hp][4Hp] -> the forward and backward fragment-ordered copies (Hp*4Hp floats each)
hipError_t launch_repack_kh(hipStream_t s, const float* Kh, float* fwd, float* bwd, int Hp);

// ---------------------------------------------------------------- XCD-local recurrence (lstm_xcd.hip), hidden size 512
// Rows are split over the 8 XCDs (ceil(B/8) each); every XCD holds a full register-resident copy of K_h and hands h_t /
// the dh partials between its own 32 CUs through its L2.  grid = 256 blocks x 256 threads; roles come from the XCC id
// plus a per-XCD ticket (tickets: 8 ints, ZERO before every launch).  Same bounded-spin / err_flag = 2 contract as the
// column-split persistent kernels.
// variants of the XCD-local kernels (same results, different schedules of the cell threads' memory traffic)
enum { XCD_DEFER_OUTPUTS = 16,      // forward: c / h / gate stores of step t are issued behind the poll of step t+1; backward: dz stores behind the drain
       XCD_NO_POLL_SLEEP = 32,      // no s_sleep between two polls of a hand-off
       XCD_CHAINS = 64,             // hidden 1024: the row groups of an XCD pair as independent chains (k_lstm_*_pair_chains)
       XCD_PROBE = 128,             // k_lstm_*_pair16: a wave polls ONE word per lane (chosen so that the wave's lanes cover every producer of its
                                    // fragments) and fetches the rest only when none of those shows the fill pattern
       XCD_LOCAL_PLAIN = 256,       // k_lstm_bwd_pair16: partials / resets between CUs of the SAME XCD stay in its L2 (plain stores)
       XCD_LATE_DRAIN = 1024,       // k_lstm_bwd_pair16: the wait for the inbox resets stands in front of the first partial store, not the MFMAs
       XCD_GROUP_STORES = 2048,     // k_lstm_bwd_xcd16: the partials of four destination tiles leave while the other four multiply
       XCD_PROBE_DELAY = 8192,      // k_lstm_fwd_pair16: x (1 ... 7) = that many times 512 clocks of sleep in front of the first probe of a wave without cell threads
       XCD_STREAM = 512 };          // k_lstm_fwd_pair16 (with XCD_PROBE): behind a successful probe the fragments are ordinary (compiler-counted) loads
                                    // consumed k step by k step under the MFMAs, checked afterwards; a miss redoes the step behind the sc1 poll
int lstm_xcd_default_variant(int B, bool forward, int Hp = 512, int rpx = 0, bool bx3 = false);
struct LstmFwdXcdArgs {
    const float* KhX;     // forward register image of K_h (launch_repack_kh_xcd)
    float* HX;            // [T+1][8][4][RG][2][64][4] hand-off buffer; index 0 = zero state, t0+1 .. t1 = 0xFF fill
    float* Z;             // [T][B][4Hp] in: x-part pre-activations (+bias); out: activated gates
    float* Cs;            // [T+1][B][Hp]
    float* Hs;            // [T+1][B][Hp]
    int* tickets;
    int* err_flag;
    int B, T, t0, t1;
    int spin_limit;
    unsigned long long* prof;   // != nullptr: instrumented build, [256 blocks][4 waves][8] tick sums per phase (RG = 2 only)
    int rpx;                    // rows per XCD; 0 = ceil(B / 8).  lstm_xcd_packed_rows(B) packs the batch on the first XCDs
    int variant;                // XCD_* bits; lstm_xcd_default_variant(B, forward) has the measured choice
    int Hp;                     // 512 (0 = 512): one copy of K_h per XCD; 1024: one copy per XCD PAIR (k_lstm_fwd_pair)
    int bx3;                    // hidden 512: KhX / HX are in the bf16-split format, run k_lstm_fwd_xcd16
    int* progress;              // bf16-split kernels only, nullptr = off: [T] counters, ZERO before the launch; progress[t] reaches
                                // lstm_xcd_active_blocks(B, rpx) when the row-major h of step t (Hs index t + 1) is in memory
                                // (write-through stores) -- what a GEMM on the other XCDs gates its row tiles on
    int progress_lag;           // diagnostics: publish this many steps later than the stores' completion requires (always 0: nothing sets it)
    int progress_every;         // publish every this many steps (0 = 1): only progress[t] with t % every == every - 1, and progress[T - 1],
                                // are counted up -- a publish is a memory operation in front of the next poll of the publishing wave
};
struct LstmBwdXcdArgs {
    const float* KhXb;    // backward register image of K_h
    float* inbox;         // [2][8][32][32][RG][16][4], every word 0xFFFFFFFF before the first launch of a pass
    float* Z;             // [T][B][4Hp] in: activated gates; out: dz
    const float* Cs;      // [T+1][B][Hp]
    float* dc;            // [B][Hp]
    const float* dH;      // [T][B][Hp]
    int* tickets;
    int* err_flag;
    int B, T, t0, t1;
    int spin_limit;
    unsigned long long* prof;
    int rpx;              // as LstmFwdXcdArgs
    int variant;          // as LstmFwdXcdArgs
    int Hp;               // as LstmFwdXcdArgs
    int bx3;              // as LstmFwdXcdArgs (KhXb in the bf16-split format, k_lstm_bwd_xcd16)
};
bool lstm_xcd_supported(int B, int Hp);        // Hp 512: up to 128 rows; Hp 1024 (one copy of K_h per XCD pair): up to 64 rows
int lstm_xcd_max_rows(int Hp);                 // 128 / 64 / 0
long long lstm_xcd_hx_floats(int B, int T, int Hp = 512, bool bx3 = false, int rpx = 0);   // bx3: for the bf16-split kernels (hidden 512); rpx: rows packed per XCD
long long lstm_xcd_inbox_floats(int B, int Hp = 512, int rpx = 0);
int lstm_xcd16_packed_rows(int B, int Hp = 512);      // bf16-split kernels: rows per XCD (hidden 1024: per XCD pair) that put B rows on the fewest (up to 16 each)
// XCD slices (hidden 1024: XCD-pair slices) of the hand-off buffer a launch with rows packed rpx per slice reads and writes -- the kernels'
// `row0 = slice * rpx >= B: return` -- out of 8 (4); rpx == 0: the rows are spread over all of them.  The forward pass refills exactly these
inline int lstm_xcd_slices(int Hp = 512) { return Hp == 1024 ? 4 : 8; }
inline int lstm_xcd_used_slices(int B, int rpx, int Hp = 512) {
    const int all = lstm_xcd_slices(Hp);
    return rpx > 0 && (B + rpx - 1) / rpx < all ? (B + rpx - 1) / rpx : all;
}
inline int lstm_xcd_active_blocks(int B, int rpx, int Hp = 512) { return (Hp == 1024 ? 64 : 32) * ((B + rpx - 1) / rpx); }     // blocks of a packed launch that own rows
long long lstm_xcd_weight_floats(int Hp = 512, bool bx3 = false);   // floats per register image
bool lstm_xcd_bx3_pays(int B, int Hp);         // the bf16-split kernels are the faster ones at this row count
int lstm_xcd_packed_rows(int B);               // rows per XCD that leave whole XCDs free without adding row groups (hidden 512)
hipError_t launch_repack_kh_xcd(hipStream_t s, const float* Kh, float* fwd, float* bwd, int Hp = 512, bool bx3 = false);
// all layers, both layouts, one launch: Kh[l] -> cf / cb (launch_repack_kh) and, where xf[l] != nullptr, xf / xb (launch_repack_kh_xcd)
constexpr int REPACK_MAX_LAYERS = 4;
struct StepIncArgs;
struct RepackAllArgs { int n; int Hp; const float* Kh[REPACK_MAX_LAYERS]; float* cf[REPACK_MAX_LAYERS]; float* cb[REPACK_MAX_LAYERS]; float* xf[REPACK_MAX_LAYERS]; float* xb[REPACK_MAX_LAYERS];
                       int bx3; /* hidden 512: the XCD images as three bf16 planes (k_lstm_*_xcd16) */
                       int mode; /* 0: both layouts, 1: the XCD / XCD-pair images only, 2: the column-split fragment copies only */ };
// inc != nullptr: thread 0 of block (0, 0) also closes the train step (step_increment_body: the repack is the last kernel of a step)
hipError_t launch_repack_kh_all(hipStream_t s, const RepackAllArgs& a, const StepIncArgs* inc = nullptr);
hipError_t launch_lstm_fwd_xcd(hipStream_t s, const LstmFwdXcdArgs& a);
hipError_t launch_lstm_bwd_xcd(hipStream_t s, const LstmBwdXcdArgs& a);

// ---------------------------------------------------------------- everything else (elementwise.hip)
// up to MULTI_MAX_OPS small memory passes in ONE launch (every pointer 16-byte aligned):
//   MULTI_FILL    dst[0 .. n) = word (32-bit pattern); cond != nullptr: only when *cond != 0 (read on the device when the launch runs)
//                 piece > 0: strided -- n = piece * count words, piece j (of `piece` words, a multiple of 4) starts at dst + j * stride
//                 (stride a multiple of 4): the pieces of a buffer a launch really uses, without a launch per piece
//   MULTI_REDUCE  dst[i] = sum_z src[z * stride + i] for i < n, slabs added in order z = 0 .. nslab - 1 (deterministic split-K);
//                 sq != nullptr: also the squared-norm partials of dst, one double per SQ_CHUNK (= sqnorm_blocks) elements, bit-equal
//                 to launch_sqnorm_partials(dst, n, sq)
//   MULTI_MEAN    *dst = sum(src[0 .. n)) / (n + 1e-12), one block, double accumulation in the order of launch_loss_reduce with one
//                 group (the mean loss of a train pass: rides in a launch that has work for the rest of the chip)
enum { MULTI_FILL = 0, MULTI_REDUCE = 1, MULTI_MEAN = 2 };
constexpr int MULTI_MAX_OPS = 16;
struct MultiOp { int kind; void* dst; const void* src; long long n; long long stride; int nslab; uint32_t word; const int* cond; double* sq;
                 const float* row_scale; int row_len; /* REDUCE without sq: dst[i] = row_scale[i / row_len] * sum (row_len % 4 == 0) */
                 long long piece; /* FILL: words per piece of a strided fill (0: one contiguous range) */ };
struct MultiOps { MultiOp op[MULTI_MAX_OPS]; int count; };
hipError_t launch_multi_op(hipStream_t s, const MultiOps& r);
// out[r][0..T) = table[idx[r]][0..T) for r < n_rows (device-resident split table -> the token staging buffer)
hipError_t launch_gather_rows(hipStream_t s, const int* table, const int* idx, int n_rows, int T, int n_songs, int* out, int* err_flag);
// p[0 .. n_words) = word (p 16-byte aligned); the step uses this instead of hipMemsetAsync so that its hipGraph holds kernel nodes only
hipError_t launch_fill32(hipStream_t s, void* p, uint32_t word, long long n_words);
// dst[0 .. n_words) = src[0 .. n_words) (both 16-byte aligned, n_words a multiple of 4): a kernel instead of hipMemcpyAsync D2D, whose
// engine (shader blit or SDMA) the runtime picks per call -- 31 us for the 78 MB of cfg-E's parameters, on the stream, every time
hipError_t launch_copy_words(hipStream_t s, void* dst, const void* src, long long n_words);
// the same, skipped on the device when *cond == 0
hipError_t launch_fill32_if(hipStream_t s, const int* cond, void* p, uint32_t word, long long n_words);
// tokens [nseq][T] (support rows then query rows) -> time-major input ids X[t][b] (start word at t=0)
// and targets Y[t][b]; sets *err_flag if any id is outside [0, vocab).
// tok_first / tok_count != nullptr (train passes): also the occurrence table of the input ids for launch_embed_grad -- first
// position (atomicMin) and count per token; both arrays [vocab + 1], (INT_MAX, 0) before the launch
hipError_t launch_token_prep(hipStream_t s, const int* support, int n_support, const int* query, int n_query,
                             int T, int vocab, int start_word, int* X, int* Y, int* err_flag, int* tok_first = nullptr, int* tok_count = nullptr);
// per logits row: lse and cross entropy against the target; dlogits != nullptr also materialises
// (softmax - onehot) * inv_n (pad columns zero) for the backward projection GEMMs
hipError_t launch_ce_rows(hipStream_t s, const float* logits, int ld, int rows, int n_vocab, const int* tgt,
                          float* lse, float* ce, float* dlogits, float inv_n);
// ---- padding-masked passes (fsmg_*_masked): a weight per row in place of the constant inv_n
// w[t * B + b] = t < len[b] ? (float)(1 / ((double)n_valid[g] + 1e-12)) : 0 and n_valid[g] = the sum of the lengths of group g = b / rows_per_group
// (B = rows_per_group * ngroups rows, lengths in [1, T]; one outside raises *err_flag |= 1 and is clamped).  Integer sums: deterministic.
hipError_t launch_row_weights(hipStream_t s, const int* len, int B, int T, int rows_per_group, int ngroups, float* w, int* n_valid, int* err_flag);
// launch_token_prep for sequences of lengths len[b] in [1, T]: positions t >= len[b] get fixed ids (input: the start word, target: 0), so
// the pass does not depend on the tokens behind a song's end; the range check covers every token all the same
hipError_t launch_token_prep_len(hipStream_t s, const int* support, int n_support, const int* query, int n_query,
                                 int T, int vocab, int start_word, int* X, int* Y, int* err_flag, int* tok_first, int* tok_count, const int* len);
// launch_ce_rows with (softmax - onehot) * w[row] (the same three kernels by ld); a row of weight 0 gets a gradient of +-0
hipError_t launch_ce_rows_w(hipStream_t s, const float* logits, int ld, int rows, int n_vocab, const int* tgt,
                            float* lse, float* ce, float* dlogits, const float* w);
// launch_ce_finish with c = w[row] / S: a row of weight 0 keeps the range check and the patch of E, crow and its row of hs_scaled are 0
hipError_t launch_ce_finish_w(hipStream_t s, const float2* part, int nparts, const int* tgt, int rows, const float* w,
                              float* E, int ld, float* lse, float* ce, float* crow, const float* hs, float* hs_scaled, int hp,
                              int* err_flag, long long* range_counter);
// out[g] = sum over the positions of group g with w != 0 of ce / (n_valid[g] + 1e-12), in launch_loss_reduce's order
hipError_t launch_loss_reduce_w(hipStream_t s, const float* ce, int T, int B, int rows_per_group, int ngroups, const float* w,
                                const int* n_valid, float* out);
// launch_gather_rows + out_len[r] = table_len[idx[r]]
hipError_t launch_gather_rows_len(hipStream_t s, const int* table, const int* table_len, const int* idx, int n_rows, int T, int n_songs,
                                  int* out, int* out_len, int* err_flag);
// what the shift-free softmax of GemmArgs::ce_store is used for: e^-60 <= S = sum_v exp(x_v) <= 1e30 (the largest logit of a row within
// about [-60, 69 - log(vocabulary)]) and exp(target logit) >= 1e-30 (its log is taken) -- E, S and c = 1 / (n S) stay normal fp32 numbers
constexpr float CE_SUM_MIN = 8.0e-27f, CE_SUM_MAX = 1.0e30f, CE_TGT_MIN = 1.0e-30f;
// Fused softmax of a train pass, second half (first: GemmArgs::ce_store): per row, from the partials -- lse, ce = lse - target logit,
// S = sum_v exp(x_v), c = inv_n / S -> crow[row]; E[row][tgt] -= S, so that (softmax - onehot) * inv_n == c * E' for the WHOLE row
// (dlogits is never written: dH = diag(c) (E' W^T), dW = (diag(c) Hout)^T E', dd = sum_r c_r E'[r]); hs_scaled[row][:] = c * hs[row][:].
// A row outside CE_SUM_MIN / CE_SUM_MAX / CE_TGT_MIN (or NaN) raises *err_flag = 2 and counts itself in *range_counter (host-mapped):
// the step is skipped and repeated on launch_ce_rows.
hipError_t launch_ce_finish(hipStream_t s, const float2* part, int nparts, const int* tgt, int rows, float inv_n,
                            float* E, int ld, float* lse, float* ce, float* crow, const float* hs, float* hs_scaled, int hp,
                            int* err_flag, long long* range_counter);
// C[m][0 .. N) *= row_scale[m] (rows of N floats, N % 4 == 0)
hipError_t launch_scale_rows(hipStream_t s, float* C, const float* row_scale, int M, int N);
// rows x nparts softmax partials (see GemmArgs::ce_part) -> ce[row] = logsumexp - target logit
hipError_t launch_ce_combine(hipStream_t s, const float2* part, int nparts, const float* tgt_logit, int rows, float* ce);
// out[g] = sum over t and b in group g of ce[t*B+b] / (T*rows_per_group + 1e-12); fixed order
hipError_t launch_loss_reduce(hipStream_t s, const float* ce, int T, int B, int rows_per_group, int ngroups,
                              float* out);
// dEmb[tok] = sum over occurrences r (increasing r) of dX[r]; dEmb must be zero-filled before
// tok_first / tok_count: the occurrence table launch_token_prep filled for this X (nullptr: every block scans for duplicates);
// the owners put their entries back to (INT_MAX, 0)
// part (with the table only): [n][Ep] scratch -- a token with more than 48 occurrences (padding, the most frequent words of real data)
// is summed in two levels, per 256-position chunk into part[first position of the chunk] and then chunk by chunk (k_embed_grad_chunks)
// sum (with part only): launch_sum_partials' work as one more block of the first launch instead of a launch of its own behind the second
struct SumPartialsArgs { const double* partials; int n; float* dst; const int* flag_src; const float* ce; int ce_n; float* loss_out; };
hipError_t launch_embed_grad(hipStream_t s, const int* X, int n, const float* dX, int Ep, float* dEmb, int* tok_first = nullptr, int* tok_count = nullptr,
                             float* part = nullptr, const SumPartialsArgs* sum = nullptr);
// partial sums of squares (double) of x[0..n) into partials[pofs .. pofs+nblocks); returns nblocks via out param
int sqnorm_blocks(long long n);
hipError_t launch_sqnorm_partials(hipStream_t s, const float* x, long long n, double* partials);

struct UpdateArgs {
    float* p; float* m; float* v; const float* g; long long n;   // flat buffers
    const double* partials; int n_partials;       // squared-norm partials of everything that counts
    const float* tail;                            // grad tail scalars (tail[0] = slices_sq, used when slices; tail[2] .. tail[5] != 0: no update)
    int use_slices;                               // add tail[0]*grad_scale^2 to the norm
    float grad_scale;                             // 1/world (g is a SUM over ranks)
    float lr, n_decay, clip;
    const long long* step;                        // global_step BEFORE this update (device)
    float* gnorm_out;                             // optional: pre-clip global norm
    const int* err_flag;                          // optional: *err_flag != 0 (a persistent step kernel gave up / a token id was out of range) -> no update
    // launch_adam_update in two launches over two ranges of the flat buffers (the second one on another stream, later): the first
    // writes publish[0..2] = (go ? 1 : 0, clip scale, alpha) from thread 0 of block 0, the second (consume != nullptr) reads them
    // instead of deriving them -- flags, tail and step counter may have moved on by then
    float* publish; const float* consume;
    // restricted form (xcd_first > 0; with consume only): blocks on an XCD below xcd_first return at once, the others draw contiguous
    // chunks of ADAM_CHUNK4 float4 from *chunk_ctr (zero before the launch) until the range is done -- the same operations on the same
    // values per element, on the XCDs a packed recurrent chain leaves free (launch_adam_update sizes the grid for them)
    int xcd_first; int* chunk_ctr;
};
constexpr int ADAM_CHUNK4 = 512;                  // float4 per drawn chunk: two per thread, eight 16-byte loads in flight
hipError_t launch_adam_update(hipStream_t s, const UpdateArgs& a);
// p <- p - a.lr * clip_by_global_norm(g): the inner-loop step of cfg-E (m, v, step, n_decay, grad_scale unused)
hipError_t launch_sgd_update(hipStream_t s, const UpdateArgs& a);

// ---------------------------------------------------------------- dynamic evaluation (dyneval.hip)
// win[0..1] = (lo, hi): the window the next window pass reads from its fixed address
hipError_t launch_set_window(hipStream_t s, int* win, int lo, int hi);
// launch_row_weights with the window [win[0], win[1]) and one group of B rows: e[b] = min(hi, len[b]), *n_valid = sum_b max(0, e[b] - lo),
// w[t * B + b] = lo <= t < e[b] ? (float)(1 / ((double)n_valid + 1e-12)) : 0, elen[b] = e[b] (the length launch_token_prep_len is given)
hipError_t launch_window_weights(hipStream_t s, const int* len, int B, int T, const int* win, float* w, int* n_valid, int* elen, int* err_flag);
// out[(row0 + b) * T + t] = -ce[t * B + b] for the positions with w[t * B + b] != 0; nothing else is written
hipError_t launch_dyneval_collect(hipStream_t s, const float* ce, const float* w, int B, int T, long long row0, float* out);
// theta_l <- theta_l - lr c g [/ (sqrt(ms / count) + eps)] + decay (theta_g - theta_l) [min(1 / decay, sqrt(ms / count) / *mean_rms)]
// c = clip > 0 ? clip / max(gnorm, clip) : 1 from the partials / tail as launch_sgd_update derives gnorm; no update when *err_flag != 0
// or tail[2..5] != 0.  decay == 0: no pull-back term (pg unread); rms == 0: ms / mean_rms unread.  n a multiple of 4.
struct DynUpdateArgs {
    float* p; const float* pg; const float* g; const float* ms; long long n;
    const double* partials; int n_partials; const float* tail; int use_slices;
    int rms; float lr, decay, eps, clip, count; const float* mean_rms;
    float* gnorm_out; const int* err_flag;
};
hipError_t launch_dyneval_update(hipStream_t s, const DynUpdateArgs& a);
// ms[i] <- ms[i] + g[i] * g[i] (fp32, two roundings), n a multiple of 4
hipError_t launch_dyneval_accumulate(hipStream_t s, float* ms, const float* g, long long n);
// *out = (float)(sum_i sqrt((double)ms[i] / count) / n_logical): fp64, fixed order; partials holds dyneval_rms_blocks(n) doubles
int dyneval_rms_blocks(long long n);
hipError_t launch_dyneval_mean_rms(hipStream_t s, const float* ms, long long n, long long count, long long n_logical, double* partials, float* out);

// ---------------------------------------------------------------- Meta-SGD: learned per-parameter inner rates (msgd.hip)
// The inner step of the MAML-style pass with a rate per element.  step = (float)(clip / max(gnorm, clip)) * lr and the conditions under
// which nothing is written are launch_sgd_update's, from the same partials / tail / error word.  Per element: st = step * alpha (one
// rounding), p -= st * g (launch_sgd_update's element line).  sum != nullptr (the train forms): sum <- fma(step, g, sum) as well -- 24 B
// per element against 16 B without it.  n a multiple of 4.
struct MsgdUpdateArgs {
    float* p; const float* g; const float* alpha; float* sum; long long n;
    const double* partials; int n_partials; const float* tail; int use_slices;
    float lr, clip; float* gnorm_out; const int* err_flag;
};
hipError_t launch_msgd_update(hipStream_t s, const MsgdUpdateArgs& a);
// ga[i] = -(g[i] * sum[i]), one rounding: the first-order gradient of the query loss with respect to the rates.  n a multiple of 4.
hipError_t launch_msgd_alpha_grad(hipStream_t s, float* ga, const float* g, const float* sum, long long n);
// clip + Adam + clamp of the rates from ga: skipped where launch_adam_update skips (err_flag, tail[2..5]);
//   gnorm = sqrt(sum of partials) * grad_scale;  scale = clip > 0 ? clip / max(gnorm, clip) * grad_scale : grad_scale
//   step size: launch_adam_update's schedule with `lr`, from *step (the launch that counts the step comes later in the stream)
//   adam_element, then alpha <- min(max(alpha, lo), hi).  partials: launch_sqnorm_partials(ga, n, partials).  n a multiple of 4.
struct MsgdAlphaArgs {
    float* alpha; float* m; float* v; const float* ga; long long n;
    const double* partials; int n_partials; const float* tail; const int* err_flag;
    float grad_scale, lr, n_decay, clip, lo, hi; const long long* step;
};
hipError_t launch_msgd_alpha_update(hipStream_t s, const MsgdAlphaArgs& a);

// ---------------------------------------------------------------- learned optimiser: a meta-learner LSTM cell per element (lopt.hip)
// The inner step of the MAML-style pass with the learned rule of include/fsmg.h "learned optimiser".  step and the conditions under which
// nothing is written are launch_sgd_update's, from the same partials / tail / error word; L_t is tail[1].  Per element (lopt_element.h):
// the gates f, i from (g, L_t, p, F, I) and phi[14] = {wF[6], bF, wI[6], bI}, then p <- f p - step (gate_scale i) g; F <- f, I <- i.
// 28 B per element.  store != nullptr (the train forms): store[j] = g[j] as well (32 B) and *sc_step = step, *sc_loss = L_t.
// n a multiple of 4.
constexpr int LOPT_MAX_BLOCKS = 2048;
struct LoptUpdateArgs {
    float* p; const float* g; float* F; float* I; float* store; float* sc_step; float* sc_loss; const float* phi; long long n;
    const double* partials; int n_partials; const float* tail; int use_slices;
    float lr, clip, gate_scale; float* gnorm_out; const int* err_flag;
};
hipError_t launch_lopt_update(hipStream_t s, const LoptUpdateArgs& a);
// Back-propagation through the K stored inner steps, one launch: per element the trajectory from p0 (theta_0) and store[t * stride + j]
// again in registers, then the walk back; G[j] <- D_0 in place, theta_out[j] = the replayed theta_K where given, and
// part[block][14] = the block's fp64 sums of the fourteen weight gradients (lopt_blocks(n) blocks).  sc: [0, 8) step_t, [8, 16) L_t.
// Nothing is written where launch_sgd_update skips.  (K + 3) x 4 B per element.  n, stride multiples of 4; K in [1, 8].
struct LoptBackpropArgs {
    float* G; const float* p0; const float* store; long long stride; const float* sc; const float* phi; float* theta_out; long long n;
    double* part; float gate_scale; const float* tail; const int* err_flag; int K;
};
hipError_t launch_lopt_backprop(hipStream_t s, const LoptBackpropArgs& a);
int lopt_blocks(long long n);
// One block.  reduce: fold[c] = (first ? 0 : fold[c]) + weight * sum over blocks of part[b][c] in fixed order, gphi[c] = (float)fold[c]
// (n_blocks == 0: the sum is 0).  Otherwise clip + Adam of phi from gphi: skipped where launch_adam_update skips;
//   gnorm = sqrt(sum gphi^2) * grad_scale;  scale = clip > 0 ? clip / max(gnorm, clip) * grad_scale : grad_scale
//   step size: launch_adam_update's schedule with `lr`, from *step;  adam_element per weight.
struct LoptPhiArgs {
    int reduce; const double* part; int n_blocks; double weight; int first; double* fold; float* gphi;
    float* phi; float* m; float* v; const float* tail; const int* err_flag; float grad_scale, lr, n_decay, clip; const long long* step;
};
hipError_t launch_lopt_phi(hipStream_t s, const LoptPhiArgs& a);

// ---------------------------------------------------------------- per-artist MAML: the fold behind an artist's query pass (tasks.hip)
// g holds the artist's gradient [n] and its tail (g + n: [0] slice sum of squares, [1] loss, [2..5] indicators), acc [n + FSMG_GRAD_TAIL]
// the running fold.  first: acc = w * g; otherwise fma(w, g, acc), written to acc or -- last -- to g.  first && last: g is left alone.
// Tail: [0] folds with w * w, [1] with w, [2..5] are 1.0f where any artist's was non-zero, the other words are left alone.
// s != nullptr (Meta-SGD): r = -(g * s), one rounding, folded by the same rule in place in ga (first && last: ga = r).
// p = p_saved in the same pass; *task_loss = g[n + 1] (may be null).  20 B per element without the rates (first: 16), 32 with them.
// n a multiple of 4.
struct TaskFoldArgs {
    float* g; float* acc; float* p; const float* p_saved; const float* s; float* ga; long long n;
    float w; int first, last; float* task_loss;
};
hipError_t launch_task_fold(hipStream_t s, const TaskFoldArgs& a);

// ---------------------------------------------------------------- dropout of the train passes (dropout.hip)
// One site of one pass: element (r, j), r a device row (t * B + b), j < W of a row of ld floats (ld a multiple of 4), is kept iff
// (word >> 8) < thr, word = output j & 3 of Philox4x32-10(counter (j >> 2, variational ? r % B : r, site, pass), key (key0, key1));
// kept elements are multiplied by scale, dropped ones and the pad columns j >= W are +0.0.  8 B per element out of place, 8 in place.
struct DropArgs {
    uint32_t key0, key1, site, pass, thr; float scale;
    int variational, B, W, ld; long long rows;
};
hipError_t launch_dropout_fwd(hipStream_t s, const DropArgs& a, const float* src, float* dst);                         // dst[r] = mask(src[r])
hipError_t launch_dropout_embed_fwd(hipStream_t s, const DropArgs& a, const float* emb, const int* ids, float* dst);   // dst[r] = mask(emb[ids[r]])
hipError_t launch_dropout_bwd(hipStream_t s, const DropArgs& a, float* g);                                             // in place
hipError_t launch_dropout_mask(hipStream_t s, const DropArgs& a, unsigned char* out);                                 // 0 / 1 bytes [rows][W]
// last kernel of a train step: counts the step (ring[step % cap] = loss, ++step) or, when *err_flag != 0 or the
// all-reduced time-out indicator tail[2] is set, tallies it in counters ([0] time-outs, [1] token-range rejections;
// host-mapped memory) and clears the flag
// handoff_dirty (the "refill the BPTT inboxes" flag) is sticky: set when *err_flag == 2, cleared only when clear_ok != 0 (the
// step ran an XCD-local BPTT pass, which did the conditional refill) and nothing timed out
struct StepIncArgs { long long* step; const float* loss_src; float loss_scale; float* ring; int ring_cap; int* err_flag; long long* counters;
                     int* handoff_dirty; int clear_ok; };
__device__ __forceinline__ void step_increment_body(const StepIncArgs& a) {
    const int e = a.err_flag != nullptr ? *a.err_flag : 0;
    if (a.handoff_dirty != nullptr) {
        if (e == 2) *a.handoff_dirty = 1;
        else if (a.clear_ok) *a.handoff_dirty = 0;
    }
    const bool peer_timeout = a.loss_src != nullptr && a.loss_src[1] != 0.0f;      // loss_src is tail[1]; tail[2] is the indicator
    const bool peer_token = a.loss_src != nullptr && a.loss_src[2] != 0.0f;        // tail[3]: some rank's batch held an out-of-range id
    const bool peer_failed = a.loss_src != nullptr && a.loss_src[3] != 0.0f;       // tail[4]: some rank's pass failed on the host before the exchange
    const bool peer_range = a.loss_src != nullptr && a.loss_src[4] != 0.0f;        // tail[5]: some rank's logits left the fused softmax's range
    if (e != 0 || peer_timeout || peer_token || peer_failed || peer_range) {
        if (a.counters != nullptr) {
            if (e == 2 || peer_timeout) a.counters[0] += 1; else if (e == 1 || peer_token) a.counters[1] += 1;
            else if (e == 4 || peer_range) a.counters[5] += 1; else a.counters[2] += 1;
            __threadfence_system();
        }
        if (a.err_flag != nullptr) *a.err_flag = 0;
        return;
    }
    const long long s = *a.step;
    if (a.ring != nullptr && a.loss_src != nullptr) a.ring[s % a.ring_cap] = *a.loss_src * a.loss_scale;
    *a.step = s + 1;
}
hipError_t launch_step_increment(hipStream_t s, const StepIncArgs& a);
// dst[0] = (float) sum of partials[0..n) (fixed order)
// ce != nullptr: also *loss_out = sum(ce[0 .. ce_n)) / (ce_n + 1e-12) -- launch_loss_reduce with one group, same bits
hipError_t launch_sum_partials(hipStream_t s, const double* partials, int n, float* dst, const int* flag_src = nullptr,
                               const float* ce = nullptr, int ce_n = 0, float* loss_out = nullptr);
// a[0 .. n_words) against b[0 .. n_words) as 32-bit words (n_words a multiple of 4, both 16-byte aligned): every differing 16-byte
// word adds 1 to *counter (host-mapped) and sets *err_flag = 2 -- the step is then skipped like a timed-out one
hipError_t launch_compare_words(hipStream_t s, const void* a, const void* b, long long n_words, int* err_flag, long long* counter);
// Do two streams run side by side?  role 0 (launched first, on stream A): one wave polls *flag for up to `realtime_ticks` of the 100 MHz
// counter and writes out[0] = 1 if it saw it set, 0 if it gave up; role 1 (on stream B): sets *flag.  Two streams that share a hardware
// queue run B behind A, and A gives up.
hipError_t launch_queue_probe(hipStream_t s, int* flag, int* out, int role, long long realtime_ticks);
// one wave for `realtime_ticks` of the 100 MHz counter: out[0] = shader-clock ticks elapsed, out[1] = real-time ticks elapsed
hipError_t launch_clock_probe(hipStream_t s, long long realtime_ticks, unsigned long long* out);
// unigram baseline (reference src/models/unigram_model.py:26-39): counts[w] += 1 per word; out[0] = -mean(log(count[w] / sum(counts))),
// out[1] = sum(counts); *out = argmax (lowest index on ties).  *err_flag |= 1 for a word outside [0, vocab)
hipError_t launch_unigram_update(hipStream_t s, const int* words, long long n, unsigned* counts, int vocab, int* err_flag);
hipError_t launch_unigram_nll(hipStream_t s, const int* words, long long n, const unsigned* counts, int vocab, float* out, int* err_flag);
hipError_t launch_unigram_argmax(hipStream_t s, const unsigned* counts, int vocab, int* out);
// batched sampling decode (decode.hip, fsmg_generate): no allocation, no synchronisation -- graph-capturable.
// One LSTM layer at one position for B rows: layer 0 (emb != nullptr) gathers x from the embedding rows tok[r * ldtok + pos];
// other layers read x [B][Hp].  h_in / h_out / c are [B][Hp]; in_dim and Hp multiples of 16.
hipError_t launch_gen_cell(hipStream_t s, const float* Kx, int in_dim, const float* Kh, const float* bias, int Hp, const float* emb, int ldemb,
                           const int* tok, int ldtok, int pos, const float* x, const float* h_in, float* h_out, float* c, int B);
// logits [B][ldl] = h [B][Hp] . W [Hp][ldw] + bias, the first ncols columns
hipError_t launch_gen_logits(hipStream_t s, const float* W, int ldw, const float* bias, int ncols, const float* h, int Hp, int B,
                             float* logits, int ldl);
// the sampling filters of fsmg_generate_filtered: repetition penalty theta (1 = off) over the distinct ids of
// tok[b][max(1, pos_out - window) .. pos_out - 1] (window 0: from 1), then min_p (0 = off), top_p (0 or >= 1 = off)
struct GenFilters {
    float top_p, min_p, theta;
    int window;
};
// per row b: Gumbel-max draw of generated token t (temperature, top_k, filters f, Philox key = seed, Philox position ctr_t >= t: t in
// a one-shot call, n_gen + t in a call that continues a decode state) -> tok[b * ldtok + pos_out], out_tok[b * num + t],
// out_lp[b * num + t] = logit - logsumexp.  f == nullptr: no filters (k_gen_pick).  ncols above 2^20 with a penalty:
// hipErrorInvalidValue (the presence bitmap of an unstaged row lives in LDS).
hipError_t launch_gen_pick(hipStream_t s, const float* logits, int ldl, int ncols, int B, float temperature, int top_k, const GenFilters* f,
                           uint64_t seed, int t, int ctr_t, int* tok, int ldtok, int pos_out, int* out_tok, float* out_lp, int num);
// constrained decoding (decode.hip, fsmg_generate_constrained): the device tables of one fsmg_constraint and the rows'
// constraint state.  Column v is allowed in (s, open) iff bias[v] > -inf, next[s * C + cls[v]] >= 0 and its slot rule holds:
// slot[v] = 0: no role; else slot k = (slot[v] & 0x7fffffff) - 1, bit 31 set: v closes k (allowed while open), clear: v opens k
// (allowed while closed).  Bit k of a row's open set is bit k & 31 of open[b * KW + (k >> 5)].
constexpr int CON_MAX_CLASSES = 64, CON_MAX_STATES = 256, CON_MAX_SLOTS = 4096;
struct ConstraintDev {
    const float* bias;            // [ncols], finite or -inf (zeros when the constraint has no bias)
    const unsigned char* cls;     // [ncols], in [0, C)
    const unsigned* slot;         // [ncols]
    const short* next;            // [S][C], in [-1, S)
    int S, C, KW;                 // KW = ceil(K / 32) <= 128
    int* state;                   // [B], in [0, S)
    unsigned* open;               // [B][KW]
    int* dead;                    // [B]
};
// launch_gen_pick under constraint c: the filtered pick on z^c (f == nullptr: no filters), then thread 0 advances row b's state
hipError_t launch_gen_pick_constrained(hipStream_t s, const float* logits, int ldl, int ncols, int B, float temperature, int top_k,
                                       const GenFilters* f, const ConstraintDev& c, uint64_t seed, int t, int ctr_t, int* tok, int ldtok,
                                       int pos_out, int* out_tok, float* out_lp, int num);
// every row's state walked over its primer tokens tok[b][1 .. P]; *err |= 1 for a token that is not allowed where it stands
hipError_t launch_constraint_advance(hipStream_t s, const ConstraintDev& c, int ncols, int B, int P, const int* tok, int ldtok, int* err);
// tok rows [start, primer[b / rows_per_primer][0..P-1]]; *err |= 1 for a primer id outside [0, vocab)
hipError_t launch_gen_primer(hipStream_t s, const int* primer, int B, int P, int vocab, int start, int* tok, int ldtok, int* err,
                             int rows_per_primer = 1);
// beam search (decode.hip, fsmg_beam_search): R = G * W rows, row r = slot r % W of group r / W; no allocation, no synchronisation.
// cum[r] = 0 for slot 0, -inf for the others
hipError_t launch_beam_init(hipStream_t s, float* cum, int R, int W);
// per row: lse and the min(W, ncols) best columns in rank order -> cand_v / cand_lp / cand_s [R][W] (s = cum[r] + lp; cand_v = -1 pads)
hipError_t launch_beam_rowtop(hipStream_t s, const float* logits, int ldl, int ncols, int R, int W, const float* cum, float* cand_s,
                              float* cand_lp, int* cand_v);
// per group: the W best of its W x W candidates -> par / htok / hlp / cum [R] and tok[r * ldtok + pos_out]
hipError_t launch_beam_select(hipStream_t s, int G, int W, int ncols, const float* cand_s, const float* cand_lp, const int* cand_v,
                              float* cum, int* tok, int ldtok, int pos_out, int* par, int* htok, float* hlp);
// constrained beam search (fsmg_beam_search_constrained): c.state / c.open / c.dead hold the R rows' constraint states.
// launch_beam_rowtop over the row's allowed set only (min(W, |Omega|) candidates, z^c = z + bias in place of the logit); a row whose
// set is empty gets launch_beam_rowtop's candidates and row_dead[r] = 1, every other row row_dead[r] = 0
hipError_t launch_beam_rowtop_constrained(hipStream_t s, const float* logits, int ldl, int ncols, int R, int W, const float* cum,
                                          const ConstraintDev& c, float* cand_s, float* cand_lp, int* cand_v, int* row_dead);
// launch_beam_select with the candidates of dead-end rows ranked below all others; new slot r also gets state_new[r] / dead_new[r] from
// its parent's row of c (advanced by the token, or at a dead-end parent unchanged with one more dead end); the new arrays are not c's
hipError_t launch_beam_select_constrained(hipStream_t s, int G, int W, int ncols, const float* cand_s, const float* cand_lp,
                                          const int* cand_v, const int* row_dead, const ConstraintDev& c, int* state_new, int* dead_new,
                                          float* cum, int* tok, int ldtok, int pos_out, int* par, int* htok, float* hlp);
// open_dst [R][KW]: each row takes its parent row's open words of c with the slot bit of its token htok[r] flipped (not c.open itself)
hipError_t launch_beam_con_reorder(hipStream_t s, int R, int W, const ConstraintDev& c, const int* par, const int* htok, const int* row_dead,
                                   unsigned* open_dst);
// h / c [L][R][Hp]: each row takes its parent row's (r / W * W + par[r])
hipError_t launch_beam_reorder(hipStream_t s, int L, int R, int W, int Hp, const int* par, const float* h_src, float* h_dst,
                               const float* c_src, float* c_dst);
// par / htok / hlp [num][R] -> out_tok / out_lp [R][num], out_score [R] = cum
hipError_t launch_beam_backtrace(hipStream_t s, int R, int W, int num, const int* par, const int* htok, const float* hlp, const float* cum,
                                 int* out_tok, float* out_lp, float* out_score);
// decode states (decode.hip, fsmg_dstate_*): no allocation, no synchronisation.
// per row b: out_lp[b * n + i] = logits[b][tok[b * ldtok + pos_tgt]] - logsumexp (the picks' lse, bitwise)
hipError_t launch_feed_logprob(hipStream_t s, const float* logits, int ldl, int ncols, int R, const int* tok, int ldtok, int pos_tgt,
                               float* out_lp, int n, int i);
// dst row i takes src row (rows ? rows[i] : i / div; rows a DEVICE array of Rd indices, one outside [0, Rs) copies nothing): h / c
// [L][R][Hp] and ntok tokens tok_src[row * ld_src + off_src ..] -> tok_dst[i * ld_dst + off_dst ..]
hipError_t launch_dstate_rows(hipStream_t s, int L, int Rd, int Rs, int Hp, const int* rows, int div, const float* h_src, float* h_dst,
                              const float* c_src, float* c_dst, const int* tok_src, int ld_src, int off_src, int* tok_dst, int ld_dst,
                              int off_dst, int ntok);
// hh / cc [n_state] = 0, tok [n_tok] = start
hipError_t launch_dstate_reset(hipStream_t s, long long n_state, float* hh, float* cc, long long n_tok, int* tok, int start);
// tokens [R][n] -> tok[r * ldtok + off + i]; *err |= 1 for an id outside [0, ncols) (stored as `start`)
hipError_t launch_dstate_tokens(hipStream_t s, const int* tokens, int R, int n, int ncols, int start, int* tok, int ldtok, int off, int* err);

// ---------------------------------------------------------------- scoring (score.hip, fsmg_score)
// Per row r = t * B + b of the time-major logits [rows = T * B][ld] (the first n_vocab columns count; ld % 4 == 0) against the target
// column tgt[r], written TRANSPOSED at [b * T + t]:
//   out_lp = z_y - (m + log(sum_v exp(z_v - m))), m the row maximum;  out_rank = #{v : z_v > z_y} + #{v < y : z_v == z_y};
//   out_ent = log S - sum_v exp(z_v - m) (z_v - m) / S, a -inf column contributing 0;  out_arg = the lowest column holding m.
// A null output is not stored.  A row with a NaN logit: NaN out_lp / out_ent, rank and argmax some column in [0, n_vocab).
// Rows of up to SCORE_REG_COLS floats are read once into registers, wider ones twice; no allocation, no synchronisation, no atomics.
constexpr int SCORE_REG_COLS = 10 * 1024;
hipError_t launch_score_rows(hipStream_t s, const float* logits, int ld, int rows, int n_vocab, const int* tgt, int B, int T,
                             float* out_lp, int* out_rank, float* out_ent, int* out_arg);

// ---------------------------------------------------------------- support-set neural cache (cache.hip, fsmg_cache_*)
// out[k * n + q] = sum_{i : vals[g][i] == y_q} exp(theta_k (d_i - d_max)) / sum_i exp(theta_k (d_i - d_max)), d_i = Q_q . keys[g][i]
// over the Mg keys of q's group g; exactly 0 when no entry holds y_q.  The host sorts the queries by group: tile j (one workgroup) holds
// up to CACHE_ATTEND_QT query ids of group tile_group[j] in slot_query[j * CACHE_ATTEND_QT ..], -1 in an empty slot.
// B == 0: query q is row q of Q (ldq floats apart) and its target tgt[q].  B > 0: q = b * T + t is row (t + 1) * B + b of Q (a pass's
// top-layer hidden states [T + 1][B][Hp], ldq = Hp) and its target tgt[t * B + b] (the pass's Y).
// Fused (no score matrix in memory), scores on the fp64 MFMA (exact products of the fp32 inputs), tail keys masked, no atomics, fixed merge order; a query's bits depend on
// its vector, its group's entries and theta alone.  No allocation, no synchronisation.
constexpr int CACHE_ATTEND_QT = 32;
constexpr int CACHE_MAX_THETA = 8;
// the exponent arithmetic every cache kernel shares (cache.hip's header comment): u = theta log2(e), and
// 2^t, t <= 0 in fp64: the fp32 exponential of the rounded exponent, corrected to first order for what the rounding dropped
constexpr double CA_LOG2E = 1.4426950408889634;
constexpr float CA_LN2 = 0.693147180559945f;
__device__ __forceinline__ double ca_exp2(double t) {
    const float hi = (float)t;
    const float lo = (float)(t - (double)hi);
    const float e = exp2f(hi);
    return (double)fmaf(e, lo * CA_LN2, e);
}
// log((1 - lambda) exp(lp) + lambda pc) in fp64, rounded once: fsmg_cache_score's mixture on the host, k_cache_mix's on the device,
// each with its own side's log / log1p / exp
__host__ __device__ inline float mix_logprob(float lp, float pc, double log1m_lambda, double log_lambda) {
    const double a = log1m_lambda + (double)lp;                         // lambda = 0: 0 + lp
    const double b = log_lambda + log((double)pc);                      // -inf at pc = 0 (and at lambda = 0)
    if (a != a || b != b) return (float)(a + b);
    const double hi = fmax(a, b), lo = fmin(a, b);
    if (hi == -INFINITY) return -INFINITY;
    return (float)(hi + log1p(exp(lo - hi)));
}
// Ragged groups: Mg is a capacity and a stride; `count` ([G], or nullptr: every group holds Mg entries) says how many
// of a group's slots exist, n_g in [1, Mg].  Every kernel that walks a group's entries walks 0 .. n_g - 1 and never scores a slot
// behind them; the group is uniform over the workgroup (or the wave), so the count is one uniform load and every branch on it is
// uniform.  With count == nullptr each kernel does what it did before the counts existed, bit for bit.
struct CacheAttendArgs {
    const float* keys;          // [G][Mg][Hp], pad units exact zeros
    const int* vals;            // [G][Mg]
    const int* count;           // [G] entries per group, or nullptr: Mg each
    int Mg, Hp;
    const float* Q; long long ldq;
    int B, T;
    const int* tgt;
    const int* slot_query;      // [n_tiles][CACHE_ATTEND_QT]
    const int* tile_group;      // [n_tiles]
    int n_tiles, n;
    float theta[CACHE_MAX_THETA]; int n_theta;      // theta >= 0
    float* out;                 // [n_theta][n]
};
size_t cache_attend_lds_bytes(int Hp);
hipError_t launch_cache_attend(hipStream_t s, const CacheAttendArgs& a);
// a pass's top-layer hidden states (Hs1: slot 1, time-major [T][B][Hp]) and targets Y [T][B] into rows r0 .. r0 + B - 1 of a cache's
// [rows][T] entries; units >= H are written as zeros
hipError_t launch_cache_fill(hipStream_t s, const float* Hs1, const int* Y, int B, int T, int H, int Hp, long long r0, float* keys,
                             int* vals);
// the compacting fill of a ragged cache: pass row b files its positions t < len[b] as entries dst[b] + t of the flat [G * Mg] entry
// array (dst[b] = g_b * Mg + the lengths of the group's earlier rows: the host's sum) and writes nothing for t >= len[b]
hipError_t launch_cache_fill_len(hipStream_t s, const float* Hs1, const int* Y, int B, int T, int H, int Hp, const int* len, const int* dst,
                                 float* keys, int* vals);

// ---- self-cache (fsmg_cache_self_attend / fsmg_cache_self_score): position t of a row attends over its group's Mg
// support entries (Mg == 0: none) and over the row's OWN entries i with t - W <= i < t, entry i = (key = the row's vector i, value =
// the row's value i); the target of position t is the row's value t.  One softmax over the union, k_cache_attend's arithmetic:
//   out[k * n_rows * T + r * T + t] = sum_{i visible, v_i = y_t} exp(theta_k (d_i - d_max)) / sum_{i visible} exp(theta_k (d_i - d_max)),
// exactly 0 when no visible entry holds y_t or none is visible at all.  Row r's vector t is V + r * vs_r + t * vs_t (Hp floats: only
// the first H are read as data, a pad unit of V may hold anything), its value t is val[r * ys_r + t * ys_t].
// One workgroup owns CACHE_ATTEND_QT consecutive positions t0 .. t0 + 31 of one row: the support keys unmasked, then the own keys
// max(0, t0 - W) .. min(t0 + 31, T - 1) - 1 in tiles of 16 under the per-(position, key) mask -- no other own key is walked.  A
// masked key is skipped, not scored as zero.  No atomics, fixed merge order: a position's bits depend on its row's vectors and values
// 0 .. t, its group's entries, theta and W alone, not on n_rows or the other rows.  No allocation, no synchronisation.
struct CacheSelfArgs {
    const float* keys;          // [G][Mg][Hp], pad units exact zeros; unused at Mg == 0
    const int* vals;            // [G][Mg]
    const int* count;           // [G] entries per group, or nullptr: Mg each
    int Mg;                     // 0: no support cache
    const int* row_group;       // [n_rows], or nullptr: all 0
    int H, Hp;
    const float* V; long long vs_r, vs_t;       // multiples of 4 floats
    const int* val; long long ys_r, ys_t;
    int n_rows, T, W;           // W >= 1
    float theta[CACHE_MAX_THETA]; int n_theta;  // theta >= 0
    float* out;                 // [n_theta][n_rows * T]
};
hipError_t launch_cache_attend_self(hipStream_t s, const CacheSelfArgs& a);

// ---- cache-conditioned generation (fsmg_cache_generate / fsmg_cache_distribution): the WHOLE mixed next-token
// distribution of R decode rows at one position, in two launches.  No allocation, no synchronisation, no atomics.
// Stage one (cache.hip), the raw scores: D[r][i] = Q_r . keys[g_r][i] for every key i < Mg of row r's group, k_cache_attend's
// arithmetic (fp32 inputs widened exactly, products on the fp64 MFMA, fp64 accumulation in one fixed k order).  The grid is
// (query tile of one group) x (chunk of CACHE_GEN_CHUNK keys), one wave each: a decode step has few rows, so the keys are what is
// spread over the chip.  The host sorts the rows by group once per call into tiles of CACHE_ATTEND_QT slots (make_tiles' layout: -1
// in an empty slot; a tile whose slot 16 is empty runs one MFMA per key fragment instead of two).  A tail key (index >= Mg in the last
// chunk) is not stored: stage two never sees it.  Every score is an accumulator element of its own: its bits depend on the row's
// vector and that key alone.
constexpr int CACHE_GEN_CHUNK = 16;
struct CacheScoresArgs {
    const float* keys;          // [G][Mg][Hp], pad units exact zeros
    const int* count;           // [G] entries per group, or nullptr: Mg each; a chunk wholly behind the count stores nothing
    int Mg, Hp;
    const float* Q; int ldq;    // row r's query: Q + r * ldq (Hp floats; the pad units finite)
    const int* slot_query;      // [n_tiles][CACHE_ATTEND_QT]
    const int* tile_group;      // [n_tiles]
    int n_tiles;
    double* D;                  // [R][Mg]
};
hipError_t launch_cache_scores(hipStream_t s, const CacheScoresArgs& a);
// Stage two (decode.hip: it shares the picks' row sweep), one workgroup per row r of group g = row_group[r]:
//   lse    the picks' logsumexp of the logits row (row_max_lse: bitwise the number k_gen_pick subtracts), lp_v = fl32(z_v - lse);
//   d_max  the exact maximum of the row's Mg scores, ONE shift S = ceil(u d_max) for every entry, w_i = ca_exp2(u d_i - S) (written
//          over D), Z = sum_i w_i over a fixed tree that depends on the group's entry count alone (Mg without counts);
//   mass   of each distinct value of the group through the cache's value index (order: the entries in stable order by value;
//          seg_beg / seg_end / seg_val: the segments of equal value, those longer than CACHE_MIX_SHORT first, n_long of n_seg): a
//          long segment is summed by one wave (lanes stride it, then a butterfly), a short one by one thread in entry order -- a
//          vocabulary of thousands gives thousands of segments of one or two entries --, either way in an order that depends on
//          the segment's length alone; pc[r][v] = fl32(mass / Z), exactly 0 for a column no entry holds;
//   z''_v  = fl32(logaddexp(log1p(-lambda) + lp_v, log(lambda) + log(pc_v))) in fp64 (mix_logprob above), over the logits
//          row in place; fl32(log1p(-lambda) + lp_v) where pc_v = 0; lambda = 0 (mix == 0): lp_v.
// A row's bits depend on its logits row, its scores, its group's values, theta and lambda alone.
constexpr int CACHE_MIX_SHORT = 32;
struct CacheMixArgs {
    float* logits; int ldl, ncols;      // [R][ldl]: z in, z'' out
    double* D; int Mg;                  // [R][Mg]: scores in, masses out (row stride Mg; the first n_g of a row exist)
    const int* count;                   // [G] entries per group, or nullptr: Mg each
    const int* row_group;               // [R]
    const int *order, *seg_beg, *seg_end, *seg_val;   // [G][Mg] each
    const int *n_seg, *n_long;          // [G]
    float* pc;                          // [R][ldl]
    float* out_lse;                     // [R] or nullptr
    double u;                           // theta log2(e)
    double log1m_lambda, log_lambda;
    int mix;                            // lambda > 0
};
hipError_t launch_cache_mix(hipStream_t s, int R, const CacheMixArgs& a);

// ---- decode-time self-cache (fsmg_cache_self_generate / fsmg_cache_self_distribution).  Row r keeps its own keys in
// own_keys[r][0 .. NP)[Hp] (pad units exact zeros); with len_r entries filed (row_len[r], or `len` for every row when row_len is
// null) it sees the last n_r = min(len_r, W) of them, entries lo_r = len_r - n_r .. len_r - 1; the value of own entry e is
// val[r * ldv + e] (generation: the token buffer shifted by one, the token that followed input e).  No allocation, no atomics.
// launch_self_file: the top layer's h_out [R][Hp] of position p into own_keys[r][p], units >= H as zeros.
hipError_t launch_self_file(hipStream_t s, const float* h_out, int R, int H, int Hp, float* own_keys, int NP, int p);
// launch_self_scores: D2[r * ldo + j] = Q_r . own_keys[r][lo_r + j], j < n_r: fp32 inputs widened exactly, every product exact in
// fp64, fp64 accumulation in one fixed order (one wave per 16 keys: lane l takes key l % 16 and the units 16 i + 4 (l / 16) .. + 3 in
// increasing i, the four partial sums of a key are added as (0 + 1) + (2 + 3)).  A score's bits depend on the two vectors alone.
struct SelfScoresArgs {
    const float* own_keys; int NP, Hp;
    const float* Q; int ldq;            // row r's query: Q + r * ldq (Hp floats, the pad units finite)
    const int* row_len; int len, W;
    double* D2; int ldo;                // ldo >= min(W, NP)
    int R;
};
hipError_t launch_self_scores(hipStream_t s, const SelfScoresArgs& a);
// launch_cache_mix_self: k_cache_mix over the UNION of the row's group's Mg support entries (Mg == 0: none; scores in D, values through
// the value index) and its n_r visible own entries (scores in D2, values in val): one exact maximum d_max and ONE shift
// S = ceil(u d_max) over both, w_i = ca_exp2(u d_i - S), Z = the sum of all of them over a tree that depends on Mg and n_r alone.
// Masses: the support segments as k_cache_mix sums them, into pm[r][v] (fp64); then the own entries, whose values change every
// step, scattered on the device without atomics: the thread of own entry j adds to pm[v_j] only if no earlier visible own entry
// holds v_j, and then the masses of j and of its later duplicates in entry order.  pc[v] = fl32(pm[v] / Z), exactly 0 for a column
// no entry holds; z'' as k_cache_mix.  An empty union (Mg == 0 and n_r == 0): pc = 0 and the row becomes lp_v = fl32(z_v - lse)
// whatever lambda is.  A row's bits depend on its logits row, its scores, its entries' values, theta and lambda alone.
struct CacheMixSelfArgs {
    CacheMixArgs m;                     // Mg == 0: D, row_group and the value index are not read
    double* D2; int ldo;                // own scores in, masses out (written over)
    const int* val; int ldv;
    const int* row_len; int len, W;
    double* pm;                         // [R][m.ldl]
};
hipError_t launch_cache_mix_self(hipStream_t s, int R, const CacheMixSelfArgs& a);

// ---- carried state of the batched passes (state.hip, fsmg_*_state).  No allocation, no synchronisation.
// launch_state_import: layer l of a decode state (h, c [B][Hp]) into slot 0 of Hs[l] / Cs[l] (row-major) and into the hand-off copy the
// layer's recurrence reads at time index 0.  kind / ng / nq / rows describe that copy:
//   STATE_HAND_HF    HF[l] index 0, fragment order [ceil(B / 16)][Hp / 16][64][4] (per-step and column-split kernels)
//   STATE_HAND_HX32  HX index 0 of the fp32 XCD-local kernels: ng weight copies (8 XCDs at hidden 512, 4 XCD pairs at 1024, 16 slices at
//                    256), nq fragments of 64 units per wave (2 / 4 / 1), rows = 4 x the row groups the launch is instantiated for
//   STATE_HAND_HX16  HX index 0 of the bf16-split kernels: ng copies (8 / 4), nq k steps of 32 units per wave (4 / 8), rows = HXR
// Pad rows and pad units of every copy are exact zeros; every word of the copy is written.
enum { STATE_HAND_NONE = 0, STATE_HAND_HF = 1, STATE_HAND_HX32 = 2, STATE_HAND_HX16 = 3 };
struct StateImportArgs {
    const float* h; const float* c;
    float* Hs0; float* Cs0;
    float* hand;
    int B, Hp, kind, ng, nq, rows;
};
hipError_t launch_state_import(hipStream_t s, const StateImportArgs& a);
// launch_token_prep_len for one block of B rows whose position 0 reads the state's pending token ctx[b * ldctx + kept] (a row of length
// 0: the start word); len (device, [B], values clamped to [0, T]) may be null = all T.  The occurrence table counts what X holds.
hipError_t launch_state_token_prep(hipStream_t s, const int* tokens, int B, int T, int vocab, int start_word, const int* len, const int* ctx,
                                   int ldctx, int kept, int* X, int* Y, int* err_flag, int* tok_first, int* tok_count);
// launch_row_weights for one group of B rows with lengths in [0, T]
hipError_t launch_state_weights(hipStream_t s, const int* len, int B, int T, float* w, int* n_valid);
// one layer of the state after the pass: h / c row b = slot len[b] of Hs / Cs ([T + 1][B][Hp]); nothing when *err_flag != 0
hipError_t launch_state_export(hipStream_t s, const float* Hs, const float* Cs, int B, int Hp, int T, const int* len, float* h, float* c,
                               const int* err_flag);
// the ring after the pass (ctx [B][ldctx], `kept` context tokens before, `keep` after); nothing when *err_flag != 0
hipError_t launch_state_export_ctx(hipStream_t s, const int* tokens, int B, int T, int vocab, const int* len, int* ctx, int ldctx, int kept,
                                   int keep, const int* err_flag);

}  // namespace fsmg
