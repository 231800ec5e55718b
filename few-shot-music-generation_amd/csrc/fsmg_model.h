// Host-side internals of libfsmg shared by the api_*.hip translation units: the model handle, its HBM layout, the helpers every
// C entry point uses.  Nothing here is exported; include/fsmg.h is the public surface, fsmg_kernels.h the launcher interface.
//   api_handle.hip    fsmg_create / fsmg_destroy, knobs, statistics
//   api_layout.hip    padded parameter layout, host <-> device tensor transfers, parameter / optimizer-state entry points
//   api_scratch.hip   activation scratch sizing, split-K policy
//   api_schedule.hip  which kernel and which order a pass takes (choose_schedule, the XCD-partitioned gate / queue), gemm()
//   api_forward.hip   forward pass builder          api_backward.hip  backward pass builder
//   api_update.hip    clip + Adam, inner-loop SGD, time-out bookkeeping, loss read-back
//   api_step.hip      train / eval / MAML-style entry points          api_comm.hip  RCCL glue (fsmg_comm_*)
//   api_unigram.hip   unigram baseline                                 api_debug.hip debug reads, timers, clock probe
//   api_decode.hip    decoding: fsmg_generate(_filtered), fsmg_beam_search, their MAML twins, fsmg_sample (one driver); decode states (fsmg_dstate_*)
//   api_score.hip     scoring of given songs: fsmg_score, fsmg_maml_score; the pass driver of every score-style call (run_passes)
//   api_cache.hip     support-set neural cache: fsmg_cache_* (build, attend, score and eval against a cache; the cache side of
//                     cache-conditioned generation, whose entry points sit beside the decode driver in api_decode.hip)
//   api_state.hip     batched passes from a carried state: fsmg_score_state, fsmg_eval_step_state, fsmg_forward_backward_state,
//                     fsmg_train_step_state (the hooks of a state pass: import, token prep, export)
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fsmg.h"
#include "fsmg_kernels.h"

namespace fsmg_host {
using namespace fsmg;
struct OpBatch;

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

constexpr int RING_CAP = 1024;
constexpr int64_t FLAT_ALIGN = 64;   // floats (256 B)
constexpr int MAX_SPLIT = 16;        // K-split cap of the GEMMs (pick_split)

struct ParamDesc {
    std::string name;
    int64_t rows, cols;     // reference shape (cols == 1 for vectors)
    int kind;               // 0 embedding, 1 kernel, 2 bias, 3 softmax_w, 4 softmax_b
    int layer;
    int64_t off, count;     // placement inside a flat buffer (floats)
};

struct TimerClass {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    int64_t launches = 0;
};

}  // namespace fsmg_host

// A decode state (fsmg_dstate_*, api_decode.hip): its own allocation, [h | c | ctx].  ctx rows are laid out as the head of a decode
// call's token rows: [start word, the last min(n_ctx, history) context tokens oldest first], the pending token the last of them.
struct fsmg_dstate_s {
    int R = 0, history = 0;
    long long n_ctx = 0, n_gen = 0;
    char* mem = nullptr;
    float *h = nullptr, *c = nullptr;   // [L][R][Hp]
    int* ctx = nullptr;                 // [R][history + 1]
    int kept() const { return (int)std::min<long long>(n_ctx, history); }
};

// A support-set cache (fsmg_cache_*, api_cache.hip): its own allocation, [keys | values].  Data only: it holds vectors and tokens and
// does not refer to the parameters that produced them.
struct fsmg_cache_s {
    int G = 0, Mg = 0, H = 0, Hp = 0;
    size_t bytes = 0;
    char* mem = nullptr;
    float* keys = nullptr;              // [G][Mg][Hp], pad units exact zeros
    int* vals = nullptr;                // [G][Mg]
    // ragged groups: entries 0 .. n_g - 1 of group g exist, the slots behind them hold zero keys and value 0 and are
    // never scored.  A uniform cache has neither array: n_g = Mg for every group, and its kernels get a null count pointer.
    int* counts = nullptr;              // device [G], inside `mem`, or nullptr
    std::vector<int> n_g;               // the host copy, empty for a uniform cache
    int entries(int g) const { return n_g.empty() ? Mg : n_g[(size_t)g]; }
    // the value index (cache-conditioned generation): per group the entries in stable order by value and the segments
    // of equal value (CacheMixArgs in fsmg_kernels.h).  An allocation of its own, built on the first call that needs it (ensure_value_index), counted in `bytes` from
    // then on, freed with the cache.
    char* idx_mem = nullptr;
    int *order = nullptr, *seg_beg = nullptr, *seg_end = nullptr, *seg_val = nullptr;   // [G][Mg] each; the long segments first
    int *n_seg = nullptr, *n_long = nullptr;                                            // [G]
};

// A constraint (fsmg_constraint_*, api_decode.hip): the device tables of ConstraintDev in one allocation, and host copies for the
// host primer's walk.
struct fsmg_constraint_s {
    int V1 = 0, S = 1, C = 1, K = 0, KW = 0, start = 0;
    char* mem = nullptr;
    float* bias = nullptr;              // device [V1]
    unsigned char* cls = nullptr;       // device [V1]
    unsigned* slot = nullptr;           // device [V1]
    short* next = nullptr;              // device [S][C]
    std::vector<float> h_bias;          // the same four on the host
    std::vector<unsigned char> h_cls;
    std::vector<unsigned> h_slot;
    std::vector<short> h_next;
};

struct fsmg_model {
    fsmg_config cfg{};
    int V = 0, V1 = 0, T = 0, E = 0, H = 0, L = 0, Ep = 0, Hp = 0, V1p = 0, G4 = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // ---- persistent state: flat fp32 buffers P (params), G (grads + tail), M, V (Adam)
    char* state = nullptr;
    bool own_state = false;
    int64_t n_flat = 0;
    float *P = nullptr, *G = nullptr, *M = nullptr, *Vv = nullptr;
    std::vector<fsmg_host::ParamDesc> params;
    int64_t off_emb = 0, off_w = 0, off_d = 0;
    std::vector<int64_t> off_kx, off_kh, off_b;
    std::vector<int> in_dim;            // padded input width of each layer (Ep or Hp)

    // ---- small device scalars
    long long* d_step = nullptr;
    int* d_err = nullptr;
    float* d_ring = nullptr;
    float* d_gnorm = nullptr;
    float* d_eval = nullptr;            // per-episode eval NLLs
    int eval_cap = 0;

    // ---- activations (scratch), sized for Bcap sequences
    int Bcap = 0;
    char* scratch = nullptr;
    int* d_tok = nullptr; int *X = nullptr, *Y = nullptr;
    std::vector<float*> Z, Hs, Cs;
    float2* ce_part = nullptr; float* tgt_logit = nullptr; int ce_nparts = 0;
    float* score_out = nullptr;         // fsmg_score: [4][T * Bcap] words -- log-prob, entropy (float), rank, argmax (int), each [b][t]
    float *dC = nullptr, *dH = nullptr, *logits = nullptr, *dlogits = nullptr, *lse = nullptr, *ce = nullptr, *dXemb = nullptr, *dXpart = nullptr;
    double* partials = nullptr;
    int partials_cap = 0;
    std::vector<float*> HF;             // fragment-ordered h per layer: [T+1][ceil(B/16)*16][Hp]
    float* dzF = nullptr;               // fragment-ordered dz ping-pong: [2][ceil(B/16)*16][4Hp]
    float* dzF_all = nullptr;           // persistent backward chain, all-gather form (where the reduce-scatter form does not apply): fragment-ordered dz of every time step
    int64_t dzfa_floats = 0;
    float* inbox = nullptr;             // persistent backward chain, reduce-scatter form: dh partial tiles [2][row tiles][P][P][64][4]
    int64_t inbox_floats = 0;
    int chain_spin_limit = 1 << 18;     // FSMG_CHAIN_SPIN_LIMIT (0 forces the timeout + fallback path: tests)
    bool retry_armed = false;           // a train step was skipped on the device and the handle has changed its schedule for the repeat: a persistent kernel
                                        // gave up (per-step launches now) or a row left the fused softmax's range (cross-entropy pass now)
    bool persist_cfg = true;            // what the configuration asked for; `persist` is what is in force right now
    int fallback_steps = 200;           // FSMG_FALLBACK_STEPS: train steps on per-step launches after a time-out, then the persistent path is tried again
    int fallback_left = 0;
    long long* host_counters = nullptr; // host-mapped tallies written by k_step_increment: [0] steps skipped after a time-out, [1] after a token-range error
    long long* d_counters = nullptr;    // the same memory as the device sees it
    long long seen_timeouts = 0, seen_token_errors = 0, seen_peer_failures = 0, seen_range_skips = 0;
    bool force_fwd_rt = false;          // FSMG_FWD_RT=1: take the all-row-tiles forward kernel wherever it applies (tests)
    bool persist = true;                // FSMG_PERSISTENT=0: one launch per time step instead of one persistent launch per chain chunk
    float* khf = nullptr;               // fragment-ordered recurrent weights: per layer fwd copy, bwd copy
    float* P_saved = nullptr;           // cfg-E: theta while the handle computes at the adapted theta'
    float* P_adapted = nullptr;         // fsmg_debug_set("keep_adapted", 1): the last theta', copied right before theta came back (tests read it:
    // per-artist MAML, allocated by the first fsmg_maml_tasks_* train call and kept until fsmg_destroy; not part of fsmg_state_bytes
    float* task_acc = nullptr;          // [n_flat + FSMG_GRAD_TAIL]: the fold of the artists so far
    float* d_task_loss = nullptr;       // [task_loss_cap]: L_n of the last tasks train call
    int task_loss_cap = 0, task_loss_n = 0;
    bool keep_adapted = false;          // fsmg_debug_read("adapted:<parameter name>")); never allocated, never written while the knob is 0
    bool have_adapted = false;
    static constexpr int MAX_TABLES = 4;
    int* table[MAX_TABLES] = {};        // device-resident packed splits [n_songs][T] (fsmg_upload_table)
    int64_t table_rows[MAX_TABLES] = {};
    int* table_len[MAX_TABLES] = {};    // the songs' lengths [n_songs] of a table that has them (fsmg_upload_table_lengths)
    int* d_idx = nullptr; int idx_cap = 0;
    // padding-masked passes (fsmg_*_masked): the lengths of the pass's sequences, the per-row loss weights and the groups' n_valid, at fixed
    // addresses in the scratch (a captured pass replays with them)
    int* d_len = nullptr;               // [Bcap] staged lengths, support rows first
    float* roww = nullptr;              // [T * Bcap] w[t * B + b] (launch_row_weights)
    int* d_nvalid = nullptr;            // [max(Bcap, 64)] per group (train pass: one group; eval batch: one per episode)
    const int* cur_len = nullptr;       // what the pass reads: d_len, or the caller's device buffer (eager pass, one contiguous array)
    bool masked_call = false;           // the call in progress is a masked one (begin_call clears it, the masked entry points set it)
    int mask_rpg = 0, mask_groups = 0;  // rows per group / groups of the masked pass in progress
    int last_mask_groups = 0;           // ... and of the last one that ran (fsmg_debug_read("n_valid"))
    // dynamic evaluation (fsmg_dyneval_*): a window pass is a masked pass whose weights come from launch_window_weights
    bool window_call = false;           // the masked pass in progress is a window pass (begin_call clears it)
    int* d_win = nullptr;               // [4] (lo, hi, -, -) at a fixed address in the scratch: a captured window pass replays with the next window
    int* d_elen = nullptr;              // [Bcap] e[b] = min(hi, len[b]) of the window pass in flight
    char* dyn_stats = nullptr;          // the gradient statistics, one allocation on first use: [ms_sum | rms partials | mean_rms]
    float* dyn_ms = nullptr;            // [n_flat] running sum of g * g, pads exact zeros
    double* dyn_part = nullptr;
    float* d_mean_rms = nullptr;
    int64_t dyn_count = 0;              // accumulated passes
    bool dyn_rms_dirty = true;          // ms_sum or count changed since d_mean_rms was computed
    float* dyn_out = nullptr; int64_t dyn_out_cap = 0;      // [R][T] scores of the call in progress
    // Meta-SGD (fsmg_msgd_*): learned per-element multipliers of the MAML-style step's inner_lr.  One allocation on the first
    // fsmg_msgd_enable, kept until fsmg_destroy: [A | AM | AV | S | GA | norm partials], the float buffers laid out like P (pads: S, GA exact 0)
    bool msgd_on = false;               // every adaptation takes launch_msgd_update in place of launch_sgd_update
    bool msgd_pending = false;          // GA belongs to the gradient that is pending (have_grads): fsmg_apply_update moves the rates with it
    char* msgd_state = nullptr;
    float *msgd_A = nullptr, *msgd_AM = nullptr, *msgd_AV = nullptr, *msgd_S = nullptr, *msgd_GA = nullptr;
    double* msgd_part = nullptr;        // [sqnorm_blocks(n_flat)] squared-norm partials of GA (the theta update's live in `partials`)
    fsmg_msgd_config msgd_cfg{};        // the scalars of the last fsmg_msgd_enable
    // learned optimiser (fsmg_lopt_*): a meta-learner LSTM cell per element in place of the inner step.  One allocation on the
    // first fsmg_lopt_enable, kept until fsmg_destroy: [Phi 14 | PM 14 | PV 14 | GPhi 14 | scalars 16 | fold 14 d | partials | F | I]; the store of
    // the train forms' support gradients is an allocation of its own (it grows with max_train_steps), the replayed theta_K another (keep_adapted)
    bool lopt_on = false;               // every adaptation takes launch_lopt_update in place of launch_sgd_update
    bool lopt_pending = false;          // GPhi belongs to the gradient that is pending (have_grads): fsmg_apply_update moves Phi with it
    char* lopt_state = nullptr;
    float *lopt_phi = nullptr, *lopt_pm = nullptr, *lopt_pv = nullptr, *lopt_gphi = nullptr, *lopt_sc = nullptr, *lopt_F = nullptr, *lopt_I = nullptr;
    double *lopt_fold = nullptr, *lopt_part = nullptr;
    float* lopt_store = nullptr; int lopt_store_steps = 0;      // [lopt_store_steps][n_flat]
    float* lopt_replay = nullptr; bool lopt_have_replay = false;
    int lopt_t = 0;                     // inner steps the adaptation in progress has taken
    bool lopt_storing = false;          // ... and whether it is a train form's (its steps are stored)
    fsmg_lopt_config lopt_cfg{};        // the scalars of the last fsmg_lopt_enable
    // dropout of the train passes (fsmg_dropout_*): masks regenerated from (seed, pass, site, row, unit), never stored
    bool drop_on = false;               // fsmg_dropout_enable / _disable
    bool drop_ever = false;             // enabled at least once (fsmg_dropout_mask / _set_pass need the scalars)
    bool drop_suppress = false;         // the gradient passes in progress are not a train form's (maml_adapt of the eval / decode forms, dynamic evaluation)
    bool drop_call = false;             // the pass in progress is a dropped one (forward_backward_core): serial, single-stream, eager
    fsmg_dropout_config drop_cfg{};
    uint64_t drop_next = 0;             // the index the next dropped pass takes
    int64_t drop_last = -1;             // ... and the one the last dropped pass took
    uint32_t drop_pass = 0;             // drop_last mod 2^32: what the kernels of the pass in progress take
    char* drop_state = nullptr;         // the masked copies, one allocation: [T * drop_cap][Ep] | L x [T * drop_cap][Hp]
    int drop_cap = 0;                   // sequences the copies hold
    int64_t drop_bytes = 0;
    std::vector<float*> drop_buf;       // [L + 1] by site
    std::vector<int> drop_lastB;        // [L + 1] rows / T of the last dropped pass that wrote the site's copy (0: none; "drop<site>")
    // carried state of a batched pass (fsmg_*_state): the pass in progress starts every layer from this decode state, reads its
    // pending token at position 0 and leaves it advanced (begin_call clears it, the state entry points set it).  Such a pass is a masked
    // pass of one group (masked_call is set with it) in the serial order: single-stream, eager
    fsmg_dstate_s* state_cur = nullptr;
    const int* state_len = nullptr;     // device lengths [R] of the state pass in progress (d_len)
    int64_t n_state_imports[4] = {};    // imports by hand-off kind (STATE_HAND_*): fsmg_debug_read("state_imports")
    int* d_gather_len = nullptr;        // ... and their lengths (the masked forms; grown and freed with d_gather)
    int* d_gather = nullptr; int64_t gather_cap = 0;     // episode rows gathered from a table for the MAML-style step (its two passes take device token buffers)
    // XCD-local recurrence (lstm_xcd.hip; hidden size 512): per layer the forward and backward register images of K_h,
    // the h hand-off buffer, the dh-partial inboxes and the per-launch ticket counters
    bool xcd = true;                    // FSMG_XCD=0: keep the column-split persistent kernels
    static constexpr int xcd_max_rows = 128;   // largest sequence count that takes the XCD-local kernels
    int dp_split = 0;                   // fsmg_config.dp_split_backward = 1 / 2: fsmg_forward_backward replays TWO graphs (forward + projection gradients | BPTT + the rest) and
                                        // records bucket 0's readiness between them, so its all-reduce runs under the second one
    int pair_mode = 2;                  // hidden size 1024 (one copy of K_h per XCD pair): 0 = column-split kernels, 1 = pair kernel forward only
                                        // (6.4 against 7.0 us per step; the backward pair kernel ties with the column-split one), 2 = both directions
    int xcd_variant = -1;               // FSMG_XCD_VARIANT: XCD_* bits for both directions (-1: lstm_xcd_default_variant)
    int xcd_variant_bwd = -1;           // FSMG_XCD_VARIANT_BWD: the backward kernels' bits alone (-1: xcd_variant / the default)
    float* khx = nullptr;
    bool xcd_bx3 = false;               // the XCD-local recurrence on the bf16 matrix pipe (k_lstm_*_xcd16 at hidden 512, k_lstm_*_pair16 at hidden 1024); one format
                                        // per handle at a time (weight images, hand-off buffer)
    bool xcd_bx3_forced = false;        // FSMG_XCD_BX3 set: the format never follows the row count of the train passes (hidden 1024: select_xcd_format)
    float* HX = nullptr; int64_t hx_floats = 0;
    float* inboxX = nullptr; int64_t inboxx_floats = 0;
    int* d_inbox_dirty = nullptr;       // device word: != 0 -> the next BPTT pass refills the inboxes first (set at creation, when the scratch moves,
                                        // and by k_step_increment after a time-out; a completed pass leaves every word reset by its reader)
    int* tickets = nullptr;             // [TICKET_LAUNCHES][8]
    static constexpr int TICKET_LAUNCHES = 64;
    int ticket_next = 0;
    int64_t n_timeouts = 0, n_persist_launches = 0, n_xcd_launches = 0, n_step_launches = 0;   // fsmg_get_stats
    bool khf_dirty = true;              // host wrote parameters since the last repack
    // the column-split fragment copies (khf) are read by the column-split / per-step kernels only: a handle whose passes take the
    // XCD-local kernels refreshes just the register images behind an update and leaves khf STALE until a pass is about to read it
    // (a big validation batch, the fallback after a time-out: ensure_cs(), api_update.hip) -- 45 -> ~17 us per update at hidden 1024
    bool lazy_cs = true;                // FSMG_LAZY_CS=0: every repack refreshes both layouts
    bool cs_stale = false;
    float* slabs = nullptr;             // split-K partial outputs of the GEMMs on the main stream
    float* arena = nullptr;             // slabs of the GEMMs whose sums are deferred into one launch (gemm(..., defer)): bump-allocated per pass
    int64_t arena_cap = 0, arena_off = 0;
    bool warned_split = false;
    // occurrence table of the input ids of a train pass (k_token_prep -> k_embed_grad): [V1] first position, [V1] count
    int* tok_first = nullptr; int* tok_count = nullptr;
    bool tok_table_open = false;        // a train-pass token_prep has been issued whose embed_grad has not (a failed call): refill before the next use
    bool last_bwd_xcd = false;          // the backward pass in flight took the XCD-local BPTT kernels (they did the conditional inbox refill)
    // eager passes: a pass on the persistent recurrent kernels is ~25 launches, which the host issues in < 0.1 ms -- replaying it
    // from a hipGraph buys nothing (measured: 534 vs 532 episodes/s at cfg-B) and costs the token staging copies, because a
    // captured token_prep cannot take the caller's pointers.  FSMG_EAGER=0: graphs wherever fsmg_config.use_graph allows.
    bool eager = true, eager_call = false;
    const int* cur_sup = nullptr; const int* cur_qry = nullptr;     // what token_prep reads: the caller's device buffers (eager) or the staging buffer
    float* colsum_slabs = nullptr;
    float* slabs2 = nullptr;            // ... and of the GEMMs on the auxiliary stream
    float* colsum_slabs2 = nullptr;
    hipStream_t probe = nullptr;        // fsmg_debug_clock_begin / _end: the shader-clock probe's own stream
    unsigned long long* d_probe = nullptr;
    hipStream_t aux = nullptr;          // second stream (DEFAULT priority since round 5: api_handle.hip pick_concurrent_aux) for what runs beside the main one
    // whether `aux` really runs beside `stream`: the runtime maps a process's streams onto GPU_MAX_HW_QUEUES (4) hardware queues per
    // priority, and two streams of one handle on the same queue run one after the other.  fsmg_create probes it (launch_queue_probe)
    // and draws another stream until the two overlap; -1: never found one (the orders that need two streams side by side are
    // switched off for the handle), else the number of streams it drew
    int aux_tries = 0;
    static constexpr int NCHUNK = 16;   // max time chunks of the overlap schedule
    static constexpr int nchunk = 8;    // chunks in use with one launch per step
    static constexpr int nchunk_persist = 4;   // ... and with the persistent step kernels (swept at cfg-B: 3-4 chunks x 2 blocks/CU)
    static constexpr int aux_blocks_persist = 2;
    static constexpr int aux_blocks_per_cu = 2;   // occupancy cap of the overlapped GEMMs; swept: 8 x 2 is best at cfg-B
    hipEvent_t ev_chunk[NCHUNK] = {};   // main -> aux (forward) / aux -> main (backward): chunk ready
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool merge_dk = true;               // dKx and dKh of a layer as one GEMM with a two-part A (FSMG_MERGE_DK=0: two GEMMs)
    hipEvent_t ev_bucket[2] = {};       // [0] softmax gradients final, [1] backward complete
    bool overlap = true;                // FSMG_OVERLAP=0 disables the two-stream schedule
    bool overlap_forced = false;        // FSMG_OVERLAP was set: no per-call decision
    bool ov_call = false;               // the decision for the call in progress (choose_schedule)
    // XCD-partitioned schedule (FSMG_XCD_OVERLAP=1; off by default: measured 385 against 388 episodes/s at cfg-B, DESIGN.md
    // section 4): the recurrence packs its rows on the first XCDs and work-queue GEMMs on the auxiliary stream take the XCDs
    // it leaves free
    int bx3 = 1;                        // FSMG_GEMM=f32 selects the fp32-MFMA GEMM, default: bf16-split (k_gemm_bx3)
    // which bf16-split kernel / how many K slabs a GEMM of this handle may take: read from the environment at creation like every
    // other knob (a process that sets them before it starts sees what it always saw; two handles of a process may differ)
    int gemm_h = 1;                     // FSMG_GEMM_H=0 / 2: the 256 x 256-tile kernel never / wherever it can run (use_h_gemm)
    int gemm_ws = 1;                    // FSMG_GEMM_WS=0 / 2: the wave-specialised kernel never / always (use_ws_gemm)
    int max_split = fsmg_host::MAX_SPLIT;   // FSMG_MAX_SPLIT=1: one K range per GEMM (pick_split)
    // GEMM launches the HOST enqueued through this handle, by kernel: [0] fp32 MFMA (k_gemm / k_gemm_staged / k_gemm_queue),
    // [1] k_gemm_bx3, [2] k_gemm_bx3w, [3] k_gemm_bx3h -- a launch captured into a hipGraph counts once, its replays do not
    // (fsmg_debug_read("gemm_kinds"))
    long long gemm_kinds[4] = {};
    bool xov = false, xov_call = false;
    bool xov_eligible = false;          // what `xov` was decided to be at creation before the second-stream probe had its say (fsmg_debug_set("reprobe_aux"))
    bool bucket0_recorded = false;      // backward() recorded ev_bucket[0] itself (two-stream / XCD-partitioned order)
    static constexpr int xov_dw_split = 4;   // K split of dW under this schedule: an item must be short against the chain it runs beside
    static constexpr int xov_pub = 6;   // the forward chain publishes every this many steps (a 256-row tile is 5.7 steps of 45 rows)
    int xov_strikes = 0;                // time-outs of passes in the XCD-partitioned order: the second one parks the schedule for this handle
    bool xov_last = false;              // the pass in flight took the XCD-partitioned order
    int xov_parts = 3;                  // FSMG_XOV_PARTS: 1 = forward pair, 2 = backward pair (dW beside the top chain), 4 = stacked layers: dK of layer l + 1
                                        // beside the BPTT chain of layer l (hidden 1024); default 3 at hidden 512, 2 at hidden 1024 (where the order is opt-in and
                                        // every part was measured to lose: api_handle.hip, profiles/r06_cfgC_xov_ab.txt)
    int* xov_prog = nullptr;            // [T] progress counters of the forward chain (LstmFwdXcdArgs::progress), the projection's gate
    // forward projection / dW: [0..1] draw counters, [2] stop flag, [3] items, [4 ..] claim words (gemm_restricted)
    static constexpr int XOV_CTL = 8192;
    int* xov_ctl = nullptr;             // [2][XOV_CTL]
    // Backward pair, hidden 512, one layer: the merged dK's items are the tail of the work list dW's clean-up launch drains
    // behind the BPTT chain -- ONE launch (k_gemm_bx3h_pair) where there were two with a kernel boundary in between; same K split, same
    // slabs, same slab sums in the same order.  FSMG_XOV_DK_TAIL=0 / fsmg_debug_set("xov_dk_tail", 0): the two launches.
    // 2 (tests only, gradients are WRONG): no clean-up launch at all, so that the claim words show what the restricted launch alone took
    int xov_dk_tail = 1;
    long long n_joint_launches = 0;     // joint clean-up launches enqueued, and the last one's item counts (fsmg_debug_read("xov_dk_tail"))
    int joint_items[2] = {0, 0};
    int64_t slab_cap = 0;
    // whole-phase hipGraphs, keyed by the shape of the call; dropped when scratch moves
    std::map<std::string, hipGraphExec_t> graphs;
    struct LaunchCounts { int64_t xcd = 0, persist = 0, step = 0; bool bwd_xcd = false; };   // bwd_xcd: what last_bwd_xcd was when the capture ended
    std::map<std::string, LaunchCounts> graph_counts;   // recurrent launches one replay of a graph stands for (fsmg_get_stats)
    // decoding (api_decode.hip): its own scratch, grown between calls after a stream sync
    char* gen = nullptr;
    size_t gen_bytes = 0;
    std::vector<fsmg_dstate_s*> dstates;   // the decode states this handle owns (fsmg_dstate_create): every entry point looks its state up here
    // support-set caches (api_cache.hip): the registry, and the attention calls' scratch (grown between calls after a stream sync)
    std::vector<fsmg_cache_s*> caches;
    std::vector<fsmg_constraint_s*> constraints;   // the constraints this handle owns (fsmg_constraint_create)
    char* cat = nullptr;
    size_t cat_bytes = 0;

    // gradient exchange inside the library (fsmg_comm_*): RCCL communicator, its stream, the event the compute stream waits on
    void* comm = nullptr; bool own_comm = false; int world = 1, rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_comm = nullptr;
    int lastB = 0;
    bool have_grads = false;
    // clip + Adam in two launches (eager passes): everything in front of softmax_w on the main stream, [softmax_w, softmax_b] on the
    // auxiliary stream beside the NEXT step's input phase (token_prep, the x-part GEMM and the fills read none of it).  The first
    // launch publishes (go, clip scale, alpha) in d_decided, the second consumes them -- it runs while k_step_increment moves the
    // step counter and clears the flags.  upd_pending: the second launch may still be in flight; settle_pending() orders the main
    // stream behind it (fsmg_host::begin_call does that for every entry point, forward() right before the first recurrent chain).
    // MEASURED AND REJECTED as a default (round 5, profiles/r05_ab_step_variants.txt, r05_step_timeline_upd_split.txt): the second
    // launch hides its 27 us, but beside it token_prep takes 9.9 instead of 4.9 us, the x-part GEMM 56.9 instead of 45.6 us, and the
    // wait in front of the first chain adds ~5 us: cfg-B -1.1 %, cfg-C -0.5 %, cfg-E -0.8 %, cfg-D +0.4 %, ref-default +0.4 %.
    bool upd_split = false;             // FSMG_UPD_SPLIT=1 / fsmg_debug_set("upd_split", 1): two launches
    bool upd_pending = false;
    hipEvent_t ev_upd_fork = nullptr, ev_upd = nullptr;
    float* d_decided = nullptr;         // [4]: go (1 / 0), clip scale, alpha, unused
    // Deferred softmax half: under the XCD-partitioned eager order (hidden 512, one layer) the fused train step launches
    // the first half only and leaves the second one NOT LAUNCHED (upd_deferred, its arguments in upd_half).  The next train pass under
    // that order launches it on the auxiliary stream right behind the x-part GEMM, restricted to the XCDs the forward chain leaves free
    // (UpdateArgs::xcd_first) -- they idle until the projection's first row tile is through its gate -- with the restricted projection
    // launch behind it in stream order; from there it is an in-flight half like upd_split's (upd_pending, ev_upd).  Anybody else goes
    // through settle_pending(), which launches a half that is still waiting unrestricted on the main stream.
    // FSMG_UPD_DEFER=0 / fsmg_debug_set("upd_defer", 0): the single in-line launch.
    bool upd_defer = true;
    bool upd_deferred = false;
    fsmg::UpdateArgs upd_half{};
    int* d_upd_ctr = nullptr;           // [4] chunk counter of the restricted launch: zeroed by the backward pass's first fills launch ...
    bool upd_ctr_zeroed = false;        // ... of this step (a restricted launch uses it once)
    long long n_upd_placed = 0, n_upd_settled = 0;      // halves launched restricted beside a forward chain / unrestricted by settle_pending (fsmg_debug_read("upd_defer"))
    // the split-K slabs of the main lane hold a GEMM's partial sums whose REDUCE op is still waiting in this batch (the XCD-partitioned
    // order's dW): gemm() flushes it before anything else writes those slabs
    fsmg_host::OpBatch* slabs_owner = nullptr;
    // self-check of the gated projection (XCD-partitioned order): the first passes of a handle compute the logits a second time on the
    // serial path and compare the words; a difference skips the step like a time-out and parks the order for this handle
    int xov_selfcheck_left = 2;         // FSMG_XOV_SELFCHECK=n
    int xov_selfcheck_every = 1000;     // FSMG_XOV_SELFCHECK_EVERY / fsmg_debug_set("xov_selfcheck_every"): one more checked pass every this many passes
                                        // under the XCD-partitioned order, for the handle's whole life (0: the first passes only)
    long long xov_passes = 0, xov_selfcheck_runs = 0;      // passes that took the order / passes that were checked (fsmg_debug_read("xov_selfcheck"))
    bool xov_selfcheck_fault = false;   // fsmg_debug_set("xov_selfcheck_fault"): compare against a buffer that is NOT the recomputed logits (tests)
    long long seen_selfcheck_mismatch = 0;
    // cross entropy writes dlogits over the logits it has just read (one 230 MB buffer instead of two at cfg-B: the pair no longer
    // exceeds the 256 MB memory-side cache); fsmg_debug_read("logits") of a train pass then returns dlogits -- FSMG_INPLACE_DLOGITS=0
    // or fsmg_debug_set("inplace_dlogits", 0) keeps both
    bool inplace_dlogits = true;
    // Fused softmax of a train pass (round 5): the projection's epilogue stores E = exp(logit) and per-slice softmax partials, a
    // per-row kernel (k_ce_finish) derives lse / ce / c_r = 1 / (n S_r), patches E[r][y_r] -= S_r and writes c_r * h_r; then
    // dH = diag(c) (E' W^T) (the scale rides in dH's slab sum), dW = (diag(c) Hout)^T E', dd = sum_r c_r E'[r] (weighted column sums in
    // the dW kernel): (softmax - onehot) / n is never materialised and the 460 MB cross-entropy pass is gone.  Taken where the
    // projection's weight gradient runs on the 256 x 256-tile kernel (use_h_gemm; the projection itself: any bf16-split kernel) and
    // dlogits are in place; a row whose sum of exp(logit) leaves [e^-60, 1e30] or whose exp(target logit) is below 1e-30 (CE_SUM_MIN /
    // CE_SUM_MAX / CE_TGT_MIN) makes the step fall back to the shifted softmax (launch_ce_rows) for good on this handle.
    // FSMG_FUSED_SOFTMAX=0 / fsmg_debug_set("fused_softmax", 0): the cross-entropy pass of rounds 1-4.
    bool fused_softmax = true;
    bool fs_call = false;               // the pass in flight takes it (forward() decides, backward() follows)
    float* Hsc = nullptr;               // [T * Bcap][Hp]: c_r * top-layer h_r (dW's A operand)
    float* crow = nullptr;              // [T * Bcap + 32]: c_r (dH's row scale, dW's column-sum weights)
    long long seen_softmax_range = 0;
    // the bandwidth-bound tail of a backward pass -- the deferred slab sums (dW / dd, the upper layers' weight gradients, dx), the mean
    // loss, k_embed_grad, the embedding-slice norm -- on the auxiliary stream BESIDE the bottom layer's weight-gradient GEMM, which is
    // issued behind dx instead of in front of it (the two do not depend on each other); the main stream waits for it right behind that
    // GEMM.  Same kernels on the same operands: same bits.  FSMG_TAIL_ASIDE=0 / fsmg_debug_set("tail_aside", 0): everything in line.
    bool tail_aside = true;
    bool side_pending = false;          // the auxiliary stream may still be reading the main lane's slabs (gemm() waits before it reuses them)
    hipEvent_t ev_side_fork = nullptr, ev_side = nullptr;
    // take_turn (api_handle.hip): recorded on this handle's stream / auxiliary stream by the NEXT handle that takes the device, which then
    // waits for them
    hipEvent_t ev_turn = nullptr, ev_turn_aux = nullptr;
    std::atomic<bool> capturing{false};      // run_graphed is between BeginCapture and EndCapture on `stream`: nobody else records on it
    std::string err;
    bool timing = false;
    std::string timing_only;
    std::map<std::string, fsmg_host::TimerClass> timers;
};

namespace fsmg_host {

extern thread_local std::string g_create_error;

inline int fail(fsmg_model* h, int code, const std::string& msg) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

// the head of every versioned config struct of include/fsmg.h: not null, the version this library was built for, zero reserved words
template <class Config>
int check_config_header(fsmg_model* h, const Config* c, const char* name, int32_t version) {
    if (!c) return fail(h, FSMG_ERR_INVALID, std::string("null ") + name);
    if (c->version != version)
        return fail(h, FSMG_ERR_INVALID, std::string(name) + ".version is " + std::to_string(c->version) + ", this library expects " +
                                             std::to_string(version));
    for (int32_t r : c->reserved)
        if (r != 0) return fail(h, FSMG_ERR_INVALID, std::string(name) + ".reserved must be zero");
    return FSMG_OK;
}

// carves one allocation into pieces that start 256 bytes aligned: take() returns a piece's offset, `off` is what has been used
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = (size_t)round_up((int64_t)(off + bytes), 256); return o; }
};

#define HIPCK(h, call)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(h, FSMG_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
    } while (0)

// roctx ranges for rocprofv3 --marker-trace timelines (FSMG_ROCTX=1): libroctx64 is looked up at run time, so the library has no
// link-time dependency on it and the ranges cost nothing when off
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        const char* e = std::getenv("FSMG_ROCTX");
        if (!e || e[0] == '0') return;
        void* lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return;
        push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
        pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (!push || !pop) push = nullptr;
    }
};
inline Roctx& roctx() { static Roctx r; return r; }
struct ScopedRange {
    bool on;
    explicit ScopedRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~ScopedRange() { if (on) roctx().pop(); }
};

struct ScopedTimer {
    fsmg_model* h; TimerClass* tc = nullptr; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(fsmg_model* h_, const char* cls) : h(h_) {
        if (!h->timing) return;
        if (!h->timing_only.empty() && h->timing_only != cls) return;
        tc = &h->timers[cls];
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { tc = nullptr; return; }
        hipEventRecord(a, h->stream);
    }
    ~ScopedTimer() {
        if (!tc) return;
        hipEventRecord(b, h->stream);
        tc->pending.emplace_back(a, b);
    }
};

inline void drain_timers(fsmg_model* h) {
    hipStreamSynchronize(h->stream);
    for (auto& kv : h->timers) {
        for (auto& pr : kv.second.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                kv.second.total_ms += ms;
                kv.second.launches += 1;
            }
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
        kv.second.pending.clear();
    }
}

// ------------------------------------------------------------------ one prologue for every C entry point that takes a handle
// begin_call: selects the handle's device and settles what an earlier call left in flight on another stream (settle_pending: the
// softmax half of the last clip + Adam update runs on the auxiliary stream beside the NEXT step's input phase, or has not been
// launched yet (upd_deferred) -- any other reader or writer of the parameters, the optimizer state or the gradient buffer must be
// ordered behind it first).  The train-step entry
// points pass keep_pending: their forward pass orders itself behind the update where it first reads the softmax parameters.
int begin_call(fsmg_model* h, bool keep_pending = false);
int settle_pending(fsmg_model* h);
// the turnstile's lock (api_handle.hip take_turn).  run_graphed holds it from `capturing = true` to `capturing = false`: take_turn
// reads the flag and records an event on the last handle's stream under the same lock, so it can never record into a capture that
// began between its check and its record (check-then-act race between threads)
std::mutex& turn_mutex();
// One handle's passes at a time per device (begin_call -> take_turn, api_handle.hip).  The persistent kernels -- recurrence chains with
// cross-CU hand-offs, gated work-queue GEMMs -- spin on CUs they hold and assume that their peers are resident; two handles of a process
// whose calls overlap on the GPU (calls return before the work is done) time-share those CUs at best and run into the hand-off time-out
// at worst (a skipped and repeated step: correct, slow).  So the first call of handle B after a call of handle A on the same device
// records what A has issued so far (both of A's streams) and makes B's streams wait for it.  A process with one handle pays a mutex
// and a pointer compare per call.  Calls on different handles from different threads AT THE SAME TIME are ordered behind the part of
// the other call that had been issued, no more.  FSMG_TURNSTILE=0: off.
#define BEGIN_CALL(h, ...)                                                           \
    do {                                                                             \
        const int rc_begin_ = fsmg_host::begin_call(h, ##__VA_ARGS__);               \
        if (rc_begin_ != FSMG_OK) return rc_begin_;                                  \
    } while (0)

// ------------------------------------------------------------------ layout (api_layout.hip)
void compute_dims(const fsmg_config& c, fsmg_model* m);
int64_t build_layout(fsmg_model* m);
int64_t state_bytes_for(int64_t n_flat);
const ParamDesc* find_param(fsmg_model* h, const char* name);
int upload_tensor(fsmg_model* h, float* flat, const char* name, const float* host, int64_t count);
int download_tensor(fsmg_model* h, const float* flat, const char* name, float* host, int64_t count);

// ------------------------------------------------------------------ scratch + split-K policy (api_scratch.hip)
int pick_split(int max_split, int64_t M, int64_t N, int64_t K, int64_t slots = 0, bool bx3 = false, int tile_mn = 0);    // max_split: the handle's cap (fsmg_model::max_split)
int ensure_scratch(fsmg_model* h, int B);
void drop_graphs(fsmg_model* h);

// A stream plus the split-K slab buffers its GEMMs may use.
struct Lane { hipStream_t s; float* slabs; float* colsum_slabs; int lds_pad; int slots; };
inline Lane main_lane(fsmg_model* h) { return Lane{h->stream, h->slabs, h->colsum_slabs, 0, gemm_block_slots()}; }
// forward-only passes (validation: many rows per step, patch step kernel) tolerate one more overlapped GEMM block
// per CU than training steps do (measured at cfg-B: eval 2862 vs 2690 episodes/s, train 290 vs 303)
inline Lane aux_lane(fsmg_model* h, bool forward_only = false, bool persistent_chain = false) {
    const int cap = std::min(4, (persistent_chain ? h->aux_blocks_persist : h->aux_blocks_per_cu) + (forward_only ? 1 : 0));
    return Lane{h->aux, h->slabs2, h->colsum_slabs2, gemm_lds_pad_for(cap), 256 * cap};
}

// ------------------------------------------------------------------ kernel / order selection (api_schedule.hip)
bool use_ws_gemm(fsmg_model* h, int amode, int bmode, const GemmArgs& g, const Lane& ln);
bool use_h_gemm(fsmg_model* h, int amode, int bmode, const GemmArgs& g, const Lane& ln);
// every GEMM launch of a handle goes through here: tallies the kernel the arguments select (fsmg_model::gemm_kinds) and launches it
inline hipError_t launch_gemm(fsmg_model* h, hipStream_t s, int amode, int bmode, const GemmArgs& g, int lds_pad = 0) {
    if (g.M <= 0 || g.N <= 0) return hipSuccess;
    const hipError_t e = fsmg::launch_gemm(s, amode, bmode, g, lds_pad);
    // (a work-queue launch that is not the 256 x 256-tile kernel's is k_gemm_queue, fp32 MFMA whatever g.bx3 says)
    if (e == hipSuccess) ++h->gemm_kinds[(g.bx3 >= 1 && g.bx3 <= 3 && !(g.xcd_first != 0 && g.bx3 != 3)) ? g.bx3 : 0];
    return e;
}

// defer != nullptr: a split-K GEMM writes its slabs into the handle's slab ARENA (bump-allocated, reset per backward pass) and
// leaves their sum as REDUCE ops in *defer instead of launching it -- the caller flushes the batch before the first reader of C
// (the five slab sums of a cfg-B backward pass were five launches of 57 us; two now).  sq: squared-norm partials of C
// (sqnorm_blocks(M * N) doubles) as a by-product of the sum; *sq_done tells the caller whether that happened.
struct OpBatch;
int gemm(fsmg_model* h, const Lane& ln, int amode, int bmode, GemmArgs g, OpBatch* defer = nullptr, double* sq = nullptr, bool* sq_done = nullptr);
#define GEMMCK(call) do { int rc_ = (call); if (rc_ != FSMG_OK) return rc_; } while (0)

// collects the small memory passes a phase needs -- pattern fills and split-K slab sums -- and issues them as one launch (flush)
// right before the first kernel that depends on them
struct OpBatch {
    MultiOps r{};
    fsmg_model* h;
    hipStream_t s;                      // where flush() launches (the main stream unless the caller moves the batch aside)
    explicit OpBatch(fsmg_model* h_) : h(h_), s(h_->stream) { r.count = 0; }
    ~OpBatch() { if (h->slabs_owner == this) h->slabs_owner = nullptr; }
    OpBatch(const OpBatch&) = delete;
    OpBatch& operator=(const OpBatch&) = delete;
    int room(int n) { return (r.count + n > MULTI_MAX_OPS) ? flush() : FSMG_OK; }
    int add(void* p, uint32_t word, long long n_words, const int* cond = nullptr) {     // cond: fill only when *cond != 0 on the device
        if (n_words <= 0) return FSMG_OK;
        const int rc = room(1); if (rc != FSMG_OK) return rc;
        MultiOp& o = r.op[r.count++];
        o = MultiOp{}; o.kind = MULTI_FILL; o.dst = p; o.word = word; o.n = n_words; o.cond = cond;
        return FSMG_OK;
    }
    // `count` pieces of `piece` words each, piece j at p + j * stride (piece and stride multiples of 4 words)
    int add_strided(void* p, uint32_t word, long long piece, long long stride, long long count) {
        if (piece <= 0 || count <= 0) return FSMG_OK;
        if (piece == stride || count == 1) return add(p, word, piece * count);
        if (((piece | stride) & 3) != 0 || piece > stride) return fail(h, FSMG_ERR_STATE, "internal: a strided fill needs piece <= stride, both multiples of 4 words");
        const int rc = room(1); if (rc != FSMG_OK) return rc;
        MultiOp& o = r.op[r.count++];
        o = MultiOp{}; o.kind = MULTI_FILL; o.dst = p; o.word = word; o.n = piece * count; o.piece = piece; o.stride = stride;
        return FSMG_OK;
    }
    // out[i] = sum over the nslab slabs (fixed order); sq: squared-norm partials of out as a by-product
    // row_scale (without sq only): out[i] = row_scale[i / row_len] * sum
    int reduce(const float* slabs, long long stride, int nslab, float* out, long long n, double* sq = nullptr, const float* row_scale = nullptr, int row_len = 0) {
        if (n <= 0) return FSMG_OK;
        // the row scale is applied by k_multi_op's float4 branch only (elementwise.hip): refuse what would take another branch and come
        // out UNSCALED instead of queueing it (today Hp % 16 == 0 keeps every caller on that branch)
        if (row_scale != nullptr && (sq != nullptr || row_len <= 0 || ((n | stride | (long long)row_len) & 3) != 0))
            return fail(h, FSMG_ERR_STATE, "internal: a row-scaled slab sum needs n, stride and row_len multiples of 4 and no squared-norm partials");
        const int rc = room(1); if (rc != FSMG_OK) return rc;
        MultiOp& o = r.op[r.count++];
        o = MultiOp{}; o.kind = MULTI_REDUCE; o.dst = out; o.src = slabs; o.stride = stride; o.nslab = nslab; o.n = n; o.sq = sq;
        o.row_scale = row_scale; o.row_len = row_len;
        return FSMG_OK;
    }
    int mean(const float* x, long long n, float* out) {       // *out = sum(x) / (n + 1e-12): one block of the launch
        if (n <= 0) return FSMG_OK;
        const int rc = room(1); if (rc != FSMG_OK) return rc;
        MultiOp& o = r.op[r.count++];
        o = MultiOp{}; o.kind = MULTI_MEAN; o.dst = out; o.src = x; o.n = n;
        return FSMG_OK;
    }
    int flush() {
        if (h->slabs_owner == this) h->slabs_owner = nullptr;      // the sums that were waiting for the main lane's slabs go out now
        if (r.count == 0) return FSMG_OK;
        HIPCK(h, launch_multi_op(s, r));
        r.count = 0;
        return FSMG_OK;
    }
};
typedef OpBatch FillBatch;

// Run `body` (a pure sequence of stream-ordered launches with call-invariant arguments) through a
// cached hipGraph: captured on first use for this key, replayed afterwards.  The ~300 launches of a
// step (one per time step and direction) then cost one hipGraphLaunch on the host.  Event timing
// needs eager launches, so graphs are bypassed while it is on.
template <class F>
int run_graphed(fsmg_model* h, const std::string& key, F&& body) {
    // hipGraph (ROCm 7.2) runs captured cross-stream branches one after the other, so the two-stream
    // schedule only overlaps with eager launches
    if (!h->cfg.use_graph || h->timing || h->ov_call || h->xov_call || h->eager_call) return body();
    auto it = h->graphs.find(key);
    if (it != h->graphs.end()) {           // a replay launches what the capture launched
        const auto& c = h->graph_counts[key];
        h->n_xcd_launches += c.xcd; h->n_persist_launches += c.persist; h->n_step_launches += c.step;
        // a replayed pass leaves the host-side facts its capture left: which BPTT family ran decides whether the update that follows
        // may clear the inbox-refill flag (the "up:...x / s" key and StepIncArgs::clear_ok)
        if (key[0] == 'f') h->last_bwd_xcd = c.bwd_xcd;
    }
    if (it == h->graphs.end()) {
        hipGraph_t graph = nullptr;
        const int64_t x0 = h->n_xcd_launches, p0 = h->n_persist_launches, s0 = h->n_step_launches;
        int rc; hipError_t e;
        {
            std::lock_guard<std::mutex> turn_lk(turn_mutex());        // nobody records on this handle's streams while they capture (take_turn)
            h->capturing.store(true);
            if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { h->capturing.store(false); return fail(h, FSMG_ERR_HIP, "hipStreamBeginCapture failed"); }
            rc = body();
            { auto& c = h->graph_counts[key]; c.xcd = h->n_xcd_launches - x0; c.persist = h->n_persist_launches - p0; c.step = h->n_step_launches - s0; c.bwd_xcd = h->last_bwd_xcd; }
            e = hipStreamEndCapture(h->stream, &graph);
            h->capturing.store(false);
        }
        if (rc != FSMG_OK) { if (graph) hipGraphDestroy(graph); return rc; }
        if (e != hipSuccess || graph == nullptr)
            return fail(h, FSMG_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (ei != hipSuccess) return fail(h, FSMG_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ei));
        it = h->graphs.emplace(key, exec).first;
    }
    HIPCK(h, hipGraphLaunch(it->second, h->stream));
    return FSMG_OK;
}

// Two-stream schedule.  The recurrent chains are latency bound (one small kernel per time step), the
// vocabulary-projection GEMMs are throughput bound, and per time chunk they are independent:
//   forward : logits + cross entropy of chunk c need h_t only for t in chunk c
//   backward: the BPTT steps of chunk c need dH only for t in chunk c; dW needs no BPTT result at all
// so the projection work runs on a low-priority auxiliary stream, forked / joined with events (inside
// the captured graph these become parallel branches).  Event timing (eager, one class at a time)
// and FSMG_OVERLAP=0 use the single-stream order.
// time-chunk boundaries of the overlap schedule: the uniform split
inline int chunk_begin(const fsmg_model* h, int c, int nch) { return (int)((int64_t)c * h->T / nch); }
inline bool use_overlap(const fsmg_model* h) { return h->ov_call && !h->timing && h->aux != nullptr && h->T >= std::max(h->nchunk, h->nchunk_persist); }

// the XCD-local kernels take this row count at this hidden size (and their buffers exist)
inline bool use_xcd(const fsmg_model* h, int B, bool backward = false) {
    if (h->Hp == 1024 && h->pair_mode < (backward ? 2 : 1)) return false;
    return h->persist && h->xcd && h->khx != nullptr && h->HX != nullptr && B <= h->xcd_max_rows && lstm_xcd_supported(B, h->Hp) &&
           lstm_xcd_hx_floats(B, h->T, h->Hp, h->xcd_bx3) <= h->hx_floats &&
           ((h->Hp == 1024 && !backward) || lstm_xcd_inbox_floats(B, h->Hp) <= h->inboxx_floats);
}
// where a train pass's cross entropy leaves dlogits (and the projection-gradient GEMMs read it)
inline float* dlogits_buf(const fsmg_model* h) { return h->inplace_dlogits ? h->logits : h->dlogits; }
// first XCD the packed recurrence leaves free
inline int xov_first_free(int B, int Hp = 512) {      // (hidden 1024: a weight copy takes an XCD pair)
    const int rpx = lstm_xcd16_packed_rows(B, Hp);
    return rpx > 0 ? (Hp == 1024 ? 2 : 1) * ((B + rpx - 1) / rpx) : 8;
}

// every XCD-local launch of a pass gets its own 8 zeroed ticket counters
inline int* next_tickets(fsmg_model* h) {
    int* t = h->tickets + 8 * (h->ticket_next % fsmg_model::TICKET_LAUNCHES);
    ++h->ticket_next;
    return t;
}

// Work-queue GEMM in two launches of k_gemm_bx3h<..., QUEUE> (GemmArgs::xcd_first): the restricted one lets the XCDs >= first
// draw items (all of them: the two launches drain one queue); the clean-up one, ordered behind the kernel that owned the other
// XCDs, lets the whole chip take what is left.  work / claim words are zeroed on the main stream before the fork.
inline int gemm_items(const GemmArgs& g) { return ((g.M + 255) / 256) * ((g.N + 255) / 256) * std::max(1, g.ksplit); }
inline bool xov_fits(const GemmArgs& g) { return 4 + gemm_items(g) <= fsmg_model::XOV_CTL; }
void choose_schedule(fsmg_model* h, int B, bool train = false);
void xov_gate(fsmg_model* h, GemmArgs& g, int B);
// hold != nullptr: the slab sums are described there instead of being queued in `defer` (the caller queues them later: gemm_queue_sums)
struct QueuedSums { const float* slabs = nullptr; const float* cslabs = nullptr; float* C = nullptr; float* colsum = nullptr; int64_t mn = 0; int S = 0; int N = 0; };
int gemm_prepare_queue(fsmg_model* h, GemmArgs& g, int split, OpBatch* defer, bool* ok, QueuedSums* hold = nullptr);
int gemm_queue_sums(OpBatch* defer, const QueuedSums& q);
// the clean-up launch of g0's queue with g1's items as its tail (GemmPairArgs); ctl: g0's queue words, 4 + both item counts of them zeroed
int gemm_cleanup_pair(fsmg_model* h, hipStream_t s, GemmArgs g0, GemmArgs g1, int* ctl);
int select_xcd_format(fsmg_model* h, int B);
int gemm_restricted(fsmg_model* h, hipStream_t s, int amode, int bmode, GemmArgs g, int first, int* ctl);
int gemm_cleanup(fsmg_model* h, hipStream_t s, int amode, int bmode, GemmArgs g, int* ctl);

// ------------------------------------------------------------------ the step pieces
// api_forward.hip
int stage_tokens(fsmg_model* h, const int32_t* support, int n_sup, const int32_t* query, int n_qry, int on_device);
int reset_tok_table(fsmg_model* h);
int token_prep(fsmg_model* h, int n_sup, int n_qry, bool train = false);
int stage_lengths(fsmg_model* h, const int32_t* support_len, int n_sup, const int32_t* query_len, int n_qry, int on_device);
// what a forward pass ends in: projection + cross entropy + loss, the bare logits (fsmg_score), or the hidden states alone (fsmg_cache_build)
enum { HEAD_LOSS = 0, HEAD_LOGITS = 1, HEAD_NONE = 2 };
int forward(fsmg_model* h, int B, int rows_per_group, int ngroups, float* loss_out, bool want_dlogits, int head = HEAD_LOSS);
GemmArgs dw_args(fsmg_model* h, int B);        // api_backward.hip: dW = Hout^T dlogits, dd = colsum(dlogits) (forward() asks which kernel it will take)
// api_backward.hip
// part 0: the whole pass; part 1: up to and including the projection gradients; part 2: the rest (see backward())
int backward(fsmg_model* h, int B, int part = 0);
// api_update.hip
int repack_recurrent_weights(fsmg_model* h, hipStream_t s, const StepIncArgs* inc, bool* inc_done);
int repack_recurrent_weights(fsmg_model* h, hipStream_t s);
int ensure_khf(fsmg_model* h);
int ensure_cs(fsmg_model* h);           // the column-split copies of K_h are current (call OUTSIDE a graph capture, before a pass that reads them)
// a pass over B sequences reads the column-split copies: its recurrence does not take the XCD-local kernels in some direction
inline bool pass_reads_cs(const fsmg_model* h, int B, bool train) {
    return !use_xcd(h, B) || (train && !use_xcd(h, B, true));
}
// may_defer: the fused single-GPU train step (the softmax half may wait for the next pass); with_rates: the Meta-SGD rates move too (update_rates)
int apply_update(fsmg_model* h, float grad_scale, bool may_defer = false, bool with_rates = false);
// api_msgd.hip.  msgd_inner_update: sgd_update with the rates (with_sum: the train forms, S collects the applied gradients);
// msgd_begin_sum: S <- 0 where an adaptation of a train form begins; msgd_rate_gradient: GA from the query pass's gradient and S, marks it
// pending; msgd_rates_due: fsmg_apply_update has rates to move; msgd_update_rates: the two launches inside apply_update
int msgd_inner_update(fsmg_model* h, float lr, bool with_sum);
int msgd_begin_sum(fsmg_model* h);
int msgd_rate_gradient(fsmg_model* h);
inline bool msgd_rates_due(const fsmg_model* h) { return h->msgd_on && h->msgd_pending && h->msgd_cfg.alpha_lr > 0.f; }
int msgd_update_rates(fsmg_model* h, float grad_scale);
// api_lopt.hip.  lopt_check_train: a train form's inner_steps against max_train_steps, before any device work; lopt_begin:
// F <- 1, I <- 0 where an adaptation begins (train: its steps are stored); lopt_inner_update: sgd_update with the learned rule;
// lopt_meta_gradient: behind a query pass -- G rewritten, GPhi folded (first / weight: the per-artist forms), marked pending;
// lopt_phi_due: fsmg_apply_update has Phi to move; lopt_update_phi: the launch inside apply_update
int lopt_check_train(fsmg_model* h, int inner_steps);
int lopt_begin(fsmg_model* h, bool train);
int lopt_inner_update(fsmg_model* h, float lr);
int lopt_meta_gradient(fsmg_model* h, bool first, double weight);
inline bool lopt_phi_due(const fsmg_model* h) { return h->lopt_on && h->lopt_pending && h->lopt_cfg.phi_lr > 0.f; }
int lopt_update_phi(fsmg_model* h, float grad_scale);
int lopt_debug_read(fsmg_model* h, const char* what, float* host, int64_t count);      // fsmg_debug_read's "lopt_*" keys
// api_dropout.hip.  drop_begin_pass: forward_backward_core, before choose_schedule -- decides drop_call and makes sure the
// masked copies hold B sequences; drop_take_index: behind the staging, where nothing host-side can refuse the pass any more -- a dropped
// pass takes its index.  drop_site_on: the site is masked in the pass in progress (its keep is below 1).
// drop_up: "layer l's output going up" -- the masked copy in a dropped pass, Hs[l] + B * Hp otherwise; drop_emb: the masked embedding
// rows [T * B][Ep] of a dropped pass (layer 0 then reads them without the gather), nullptr otherwise.  drop_forward_site: the site's
// forward launch; drop_backward_site: the same factors, in place, on the gradient g [T * B][ld] that flows back through the site.
int drop_begin_pass(fsmg_model* h, int B);
void drop_take_index(fsmg_model* h);
inline float drop_keep(const fsmg_model* h, int site) { return site == 0 ? h->drop_cfg.keep_input : h->drop_cfg.keep_output; }
inline bool drop_site_on(const fsmg_model* h, int site) { return h->drop_call && drop_keep(h, site) < 1.0f; }
inline const float* drop_up(const fsmg_model* h, int l, int B) {
    return drop_site_on(h, l + 1) ? h->drop_buf[l + 1] : h->Hs[l] + (size_t)B * h->Hp;
}
inline const float* drop_emb(const fsmg_model* h) { return drop_site_on(h, 0) ? h->drop_buf[0] : nullptr; }
int drop_forward_site(fsmg_model* h, int site, int B);
int drop_backward_site(fsmg_model* h, int site, int B, float* g);
void drop_destroy(fsmg_model* h);
// api_state.hip, the hooks of a state pass (fsmg_model::state_cur != nullptr):
// state_token_prep: token_prep's launches -- one group's weights with lengths in [0, T], the pending token at position 0
// state_import: forward(), per layer in place of the zero fills of slot 0 (xcd: the layer's chain takes the XCD-local kernels)
// state_export: behind the pass's last reader of Hs / Cs and in front of whatever clears the error word: slot len[b] and the ring
// state_train_pass (api_step.hip): forward + backward (+ update) of the state's rows, the masked train forms' contract
int state_token_prep(fsmg_model* h, int B, bool table);
int state_import(fsmg_model* h, int l, int B, bool xcd);
int state_export(fsmg_model* h, int B);
int state_train_pass(fsmg_model* h, int R, const int32_t* tokens, const int32_t* len, int on_device, bool with_update, float* loss);
int place_deferred_half(fsmg_model* h, int xcd_first);     // forward(): the waiting half on the auxiliary stream, on the XCDs >= xcd_first
int sgd_update(fsmg_model* h, float lr);
int save_theta(fsmg_model* h);
int restore_theta(fsmg_model* h);
int keep_theta_prime(fsmg_model* h);      // before every restore_theta: P -> P_adapted where fsmg_debug_set("keep_adapted", 1) asks for it
void on_timeout(fsmg_model* h);
void on_softmax_range(fsmg_model* h);
inline bool is_retry(int rc) { return rc == FSMG_ERR_TIMEOUT || rc == FSMG_ERR_SOFTMAX_RANGE; }
// ---- the train / MAML drivers (api_step.hip; DESIGN.md "cfg-E", 20, 22, 23, 27), shared with api_tasks.hip, api_dyneval.hip, api_state.hip
// and the decode / score entry points at theta'
int validate_shape(fsmg_model* h, int N, int K, int Q);
int validate_masked_args(fsmg_model* h, const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t on_device);
// the call in progress is a padding-masked pass over `groups` groups of `rows_per_group` sequences (behind begin_call, which clears the flag)
inline void begin_masked(fsmg_model* h, int rows_per_group, int groups) {
    h->masked_call = true; h->mask_rpg = rows_per_group; h->mask_groups = groups;
}
// Where a MAML call's rows are once its arguments are checked (and, for a table form, gathered): [N * K][T] support rows, [N * Q][T] query
// rows, their lengths where the call is a padding-masked one.  Artist n's support rows start at sup + n * K * T, its lengths at slen + n * K.
struct Episode {
    const int32_t *sup = nullptr, *qry = nullptr, *slen = nullptr, *qlen = nullptr;
    int32_t N = 0, K = 0, Q = 0;
    int on_device = 0;
    bool masked = false;
    Episode artist(int n, int T) const {        // artist n alone, as an episode of one
        Episode a = *this;
        a.N = 1; a.sup += (size_t)n * K * T; a.qry += (size_t)n * Q * T;
        if (masked) { a.slen += (size_t)n * K; a.qlen += (size_t)n * Q; }
        return a;
    }
};
// the token form: the rows are where the caller says, masked iff it gave lengths
inline Episode token_episode(const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K,
                             int32_t Q, int on_device) {
    Episode e;
    e.sup = support; e.qry = query; e.slen = support_len; e.qlen = query_len; e.N = N; e.K = K; e.Q = Q;
    e.on_device = on_device; e.masked = support_len != nullptr;
    return e;
}
// the table form: the rows under the indices (with_len: and their lengths; a table without them: FSMG_ERR_STATE) are gathered ONCE into
// d_gather / d_gather_len and every pass of the call reads them there
int gather_episode(fsmg_model* h, int32_t table_id, bool with_len, const int32_t* support_idx, const int32_t* query_idx, int32_t N, int32_t K,
                   int32_t Q, Episode* e);
// table_id >= 0: gather_episode with support / query as the indices; otherwise token_episode
int locate_episode(fsmg_model* h, int32_t table_id, bool with_len, const int32_t* support, const int32_t* query, const int32_t* support_len,
                   const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int on_device, Episode* e);
// forward + backward over the N * R rows [N * R][T] as support-position rows of one group; len != nullptr: the padding-masked pass over
// their lengths.  Its own prologue (begin_call with keep_pending), masked_call cleared behind it.
int rows_pass(fsmg_model* h, const int32_t* rows, const int32_t* len, int32_t N, int32_t R, int32_t on_device);
// the dynamic-evaluation driver's pass: rows_pass over host rows with the loss weights on [lo, min(hi, len[b])) only, never dropped
int window_rows_pass(fsmg_model* h, const int32_t* rows, const int32_t* len, int32_t n, int lo, int hi);
// theta saved, `inner_steps` clipped-SGD (or Meta-SGD) steps on the episode's support rows.  train: a train form's adaptation (dropout
// applies; with Meta-SGD S collects the applied steps)
int maml_adapt(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, bool train);
// the error word the passes so far have left, read back and cleared; a time-out switches the handle to per-step launches and is
// reported as FSMG_ERR_TIMEOUT
int adapt_flag(fsmg_model* h);
// The end of an adaptation, whatever happened in it: masked_call and window_call cleared, theta' kept where the debug knob asks for it,
// theta back, no gradient pending.  Returns the first failure of its own.
int end_adaptation(fsmg_model* h);
// adapt(), body() at the adapted parameters, end_adaptation; where the adaptation ran skipped steps (a time-out: the handle has switched
// to per-step launches) all three once more
int at_adapted_theta(fsmg_model* h, const std::function<int()>& adapt, const std::function<int()>& body);
// the three MAML calls behind their entry points' argument checks
int maml_forward_backward(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr);
int maml_step(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, float* loss);
int maml_eval(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, float* nll);
// adapt on the support rows like maml_eval, run `at_theta_prime` there, restore theta whatever happened (the MAML decode and score
// entry points in api_decode.hip / api_score.hip)
int with_adapted_theta(fsmg_model* h, const int32_t* support, int32_t n_support_rows, int32_t inner_steps, float inner_lr,
                       int32_t support_on_device, const std::function<int()>& at_theta_prime, const int32_t* support_len = nullptr,
                       bool masked = false);      // masked: every inner step over the positions t < support_len[b] only
// the episode-parallel step with the exchange inside the library: forward_backward(), all-reduce, clip + Adam (1 / world)
int dp_train_step(fsmg_model* h, float* loss, const std::function<int()>& forward_backward);
// forward_backward() and the outer update of a MAML-style step: dp_train_step with a communicator, otherwise fsmg_apply_update(1) and,
// after a time-out, both once more on per-step launches with the masks of the passes they repeat
int step_with_update(fsmg_model* h, float* loss, const std::function<int()>& forward_backward);
// api_dyneval.hip: adapt on the support stream by dynamic evaluation (nothing reported), run `at_theta_l` there, restore theta whatever
// happened -- with_adapted_theta's twin (fsmg_dyneval_generate, api_decode.hip)
int with_dyneval_theta(fsmg_model* h, const fsmg_dyneval_config* c, const int32_t* support, const int32_t* support_len, int32_t n_support_rows,
                       const std::function<int()>& at_theta_l);
int poll_skipped(fsmg_model* h);
int report(fsmg_model* h, int what);
int check_tokens_and_read(fsmg_model* h, const float* d_src, float scale, float* host_out, int n, bool train_tail = false);
int after_update(fsmg_model* h, float grad_scale, float* loss);
// api_score.hip: what the score-style calls share (fsmg_score, fsmg_cache_build, fsmg_cache_score and their variants)
// The R rows of `tokens` ([R][T], on the host or the device) in passes of P rows.  Per pass of B rows from row r0: choose_schedule,
// one stream for the call (ov_call = false), ensure_cs where the pass reads the column-split copies, stage_tokens; launch(r0, B)
// enqueues the pass's launches and read_back(r0, B) its device-to-host copies; the error word comes back behind them with the
// pass's one stream synchronisation and is cleared.  After a time-out the handle has switched to per-step launches and the pass is
// repeated that way, at most once.
int run_passes(fsmg_model* h, const int32_t* tokens, int R, int P, int on_device, const std::function<int(int, int)>& launch,
               const std::function<int(int, int)>& read_back);
int check_host_tokens(fsmg_model* h, const int32_t* tokens, size_t n);      // every id in [0, input_size), before any device work
// out[r] = -mean of logprob[r][t0 .. t1) over R rows of T: fp64, increasing t, rounded once -- bitwise recomputable from the log-probs
void row_nll(const float* logprob, int R, int T, int nll_first, int nll_count, float* out);
// the same over the scored positions t < len[r] of the window; NaN where the window holds none
void row_nll_masked(const float* logprob, int R, int T, int nll_first, int nll_count, const int32_t* len, float* out);
// host lengths [n] of a *_masked scoring / cache call: non-null and every value in [1, max_len], before any device work
int check_host_lengths(fsmg_model* h, const int32_t* len, size_t n);
// api_decode.hip / api_cache.hip: what cache-conditioned generation shares between the decode driver and the cache
int gen_reserve(fsmg_model* h, size_t bytes);              // h->gen holds at least `bytes`: grown between calls, after a stream sync
fsmg_cache_s* find_cache(fsmg_model* h, fsmg_cache c);     // the cache if this handle owns it, else nullptr with the error set
// One call's cache side: the rows sorted by group into tiles once, the kernels' scratch inside the caller's block of h->gen.
struct CacheGen {
    const fsmg_cache_s* c = nullptr;
    float theta = 0.f, lambda = 0.f;
    int R = 0, ldl = 0;
    std::vector<int> slot_query, tile_group, row_group;     // host copies: alive until the stream has been synchronised
    int *d_slot_query = nullptr, *d_tile_group = nullptr, *d_row_group = nullptr;
    double* D = nullptr;                                    // [R][Mg]
    float* pc = nullptr;                                    // [R][ldl]
    // the self-cache beside it (W > 0; c may then be null: no support entries): NP positions of own keys per row, ldo = min(W, NP)
    int W = 0, NP = 0, ldo = 0, Hp = 0;
    bool raw = false;                                       // fsmg_cache_self_distribution: per-row lengths and values from the host
    float* own_keys = nullptr;                              // [R][NP][Hp]
    double* D2 = nullptr;                                   // [R][ldo]
    double* pm = nullptr;                                   // [R][ldl]
    int *d_len = nullptr, *d_val = nullptr;                 // raw: [R], [R][NP]
};
// fsmg_cache_self_generate / _distribution: cache_gen_check (cache may be null) plus the self config and the scratch bounds
int cache_self_gen_check(fsmg_model* h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                         const int32_t* group, int64_t R, int64_t NP, bool raw, CacheGen* cg);
// position p of a generate call: the top layer's h_out [R][Hp] becomes own entry p of every row
int cache_self_file(fsmg_model* h, const CacheGen& cg, const float* h_out, int p);
// the launches at one position over the union: len own entries filed per row (raw: cg.d_len), own entry e of row r holds val[r * ldv + e]
int cache_self_step(fsmg_model* h, const CacheGen& cg, int len, const float* Q, float* logits, const int* val, int ldv, float* out_lse);
// the argument checks (no device work): config, cache against the handle, group ids, the R * Mg limit; fills cg's host side
int cache_gen_check(fsmg_model* h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const int32_t* group, int64_t R, CacheGen* cg);
int ensure_value_index(fsmg_model* h, fsmg_cache_s* c);    // outside the token loop: allocates and synchronises on first use
size_t cache_gen_bytes(const fsmg_model* h, const CacheGen& cg);
int cache_gen_place(fsmg_model* h, CacheGen& cg, char* base);       // the pointers into `base` (cache_gen_bytes of it), tiles uploaded
// the two launches at one position: the rows' queries Q [R][Hp], their logits [R][ldl] overwritten with z''
int cache_gen_step(fsmg_model* h, const CacheGen& cg, const float* Q, float* logits, float* out_lse);
void free_cache(fsmg_cache_s* c);
// api_comm.hip
int exchange_gradients(fsmg_model* h);
void comm_destroy(fsmg_model* h);       // fsmg_destroy's share: communicator, its stream and event

}  // namespace fsmg_host
