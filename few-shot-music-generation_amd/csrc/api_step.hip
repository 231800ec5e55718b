// Train / eval / MAML-style step entry points and the device-resident episode table; the drivers every adapting call shares (rows_pass,
// maml_adapt, end_adaptation, at_adapted_theta, step_with_update; the Episode a MAML call runs on: DESIGN.md 28).
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); every kernel lives in gemm.hip / lstm_*.hip / elementwise.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

int validate_shape(fsmg_model* h, int N, int K, int Q) {
    if (N <= 0 || K < 0 || Q < 0 || (int64_t)N * (K + Q) <= 0 || (int64_t)N * (K + Q) > (1 << 20))
        return fail(h, FSMG_ERR_INVALID, "bad episode shape N/K/Q");
    return FSMG_OK;
}

// forward + backward of one episode whose tokens `stage` puts into the handle's staging buffer ([n_sup + n_qry][T], support rows first)
// with_update: the clip + Adam update (grad_scale 1) rides in the same captured graph -- the single-GPU train step; a
// gradient exchange between the two halves (episode-parallel training) needs them as separate calls
template <class Stage>
int forward_backward_core(fsmg_model* h, int32_t N, int32_t K, int32_t Q, Stage&& stage, bool with_update = false) {
    int rc = validate_shape(h, N, K, Q);
    if (rc != FSMG_OK) return rc;
    const int B = N * (K + Q);
    if (h->fallback_left > 0 && --h->fallback_left == 0 && h->persist != h->persist_cfg) {   // try the persistent path again
        h->persist = h->persist_cfg;
        drop_graphs(h);
    }
    if ((rc = ensure_scratch(h, B)) != FSMG_OK) return rc;
    if ((rc = select_xcd_format(h, B)) != FSMG_OK) return rc;
    if ((rc = drop_begin_pass(h, B)) != FSMG_OK) return rc;
    struct DropScope { fsmg_model* m; ~DropScope() { m->drop_call = false; } } drop_scope{h};      // whatever way the pass ends, it is over
    choose_schedule(h, B, true);
    h->xov_last = h->xov_call;
    // an eager pass orders itself behind a pending update half inside forward(); a pass that is captured or replayed cannot hold
    // a wait on an event recorded outside the graph
    if (!h->eager_call && (rc = settle_pending(h)) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    if (pass_reads_cs(h, B, true) && (rc = ensure_cs(h)) != FSMG_OK) return rc;
    if (h->tok_table_open && (rc = reset_tok_table(h)) != FSMG_OK) return rc;     // a pass that never reached its embed_grad
    h->tok_table_open = true;
    if ((rc = stage()) != FSMG_OK) return rc;
    drop_take_index(h);                 // (a call refused up to here has used up no pass index)
    const int n_sup = N * K, n_qry = N * Q;
    h->bucket0_recorded = false;
    // (a padding-masked pass has launches of its own -- the row weights, the weighted cross entropy, the masked loss: its own graphs)
    const std::string shape_key = std::to_string(n_sup) + ":" + std::to_string(n_qry) + (h->masked_call ? (h->window_call ? ":w" : ":m") : "");      // (a window pass: the weights' kernel differs)
    if (h->dp_split && !with_update) {
        // episode-parallel order: bucket 0 (softmax gradients, 56 % of the bytes at cfg-B) is final when the first graph ends and
        // travels while the second one (BPTT, weight / input gradients, embedding gradient) runs
        rc = run_graphed(h, "fb1:" + shape_key, [&]() -> int {
            int r = token_prep(h, n_sup, n_qry, true);
            if (r == FSMG_OK) r = forward(h, B, B, 1, h->G + h->n_flat + 1, true);
            if (r == FSMG_OK) r = backward(h, B, 1);
            return r;
        });
        if (rc != FSMG_OK) return rc;
        if (!h->bucket0_recorded) { HIPCK(h, hipEventRecord(h->ev_bucket[0], h->stream)); h->bucket0_recorded = true; }
        rc = run_graphed(h, "fb2:" + shape_key, [&]() -> int {
            int r = backward(h, B, 2);
            if (r == FSMG_OK && h->state_cur != nullptr) r = state_export(h, B);
            return r;
        });
    } else {
        rc = run_graphed(h, (with_update ? "fbu:" : "fb:") + shape_key, [&]() -> int {
            int r = token_prep(h, n_sup, n_qry, true);
            if (r == FSMG_OK) r = forward(h, B, B, 1, h->G + h->n_flat + 1, true);
            if (r == FSMG_OK) r = backward(h, B);
            // a state pass: the state advances behind the last reader of Hs / Cs and in front of the update, whose
            // k_step_increment clears the error word the export looks at -- a skipped step leaves the state where it was
            if (r == FSMG_OK && h->state_cur != nullptr) r = state_export(h, B);
            if (r == FSMG_OK && with_update) r = apply_update(h, 1.0f, true);
            return r;
        });
    }
    if (rc != FSMG_OK) return rc;
    h->tok_table_open = false;          // (a replayed graph ran its embed_grad too)
    // bucket readiness for an overlapped gradient exchange: with the two-stream (eager) schedule bucket 0 was
    // recorded right behind the dW GEMM on the aux stream; a replayed graph finishes as a whole
    // (the fused single-GPU step has applied its update already: nobody waits for a bucket, and two event records between
    // consecutive steps are ~10 us of queue time)
    if (!with_update) {
        if (!h->bucket0_recorded) HIPCK(h, hipEventRecord(h->ev_bucket[0], h->stream));
        HIPCK(h, hipEventRecord(h->ev_bucket[1], h->stream));
    }
    h->lastB = B;
    h->have_grads = !with_update;
    h->msgd_pending = false;            // (a rate gradient belongs to the pass it was formed from: msgd_rate_gradient sets it behind the query pass)
    h->lopt_pending = false;            // (and so does a GPhi: lopt_meta_gradient)
    return FSMG_OK;
}

// the episode-parallel step with the exchange inside the library: forward + backward, all-reduce, clip + Adam (1 / world)
int dp_train_step(fsmg_model* h, float* loss, const std::function<int()>& forward_backward) {
    const uint64_t drop_p0 = h->drop_next;      // a repeated step draws the masks of the passes it repeats
    for (int attempt = 0; attempt < 2; ++attempt) {
        h->drop_next = drop_p0;
        int rc = forward_backward();
        int local_rc = FSMG_OK; std::string local_msg;
        if (rc != FSMG_OK) {
            // A failure on THIS rank's host (an allocation, a launch) must not leave the peers blocked in ncclAllReduce: join the
            // collectives with the "this rank's gradients are garbage" indicator raised (tail[4]; summed like the time-out and
            // token-range indicators), so that every rank skips the update and every rank's step ends -- then report the failure.
            local_rc = rc; local_msg = h->err;
            if (launch_fill32(h->stream, h->G + h->n_flat + 4, 0x3f800000u, 1) != hipSuccess) return local_rc;     // 1.0f
            if (hipEventRecord(h->ev_bucket[0], h->stream) != hipSuccess || hipEventRecord(h->ev_bucket[1], h->stream) != hipSuccess) return local_rc;
            h->have_grads = true;
        }
        rc = exchange_gradients(h);
        const float scale = 1.0f / (float)h->world;
        if (rc == FSMG_OK) {
            uint32_t bits; std::memcpy(&bits, &scale, 4);
            rc = run_graphed(h, "up:" + std::to_string(bits) + (h->last_bwd_xcd ? "x" : "s"), [&]() -> int { return apply_update(h, scale); });
        }
        if (rc == FSMG_OK) rc = after_update(h, scale, loss);
        if (local_rc != FSMG_OK) { h->err = local_msg; return local_rc; }
        // a time-out on ANY rank travelled in the reduced tail: every rank skipped the update, reports it here and repeats the
        // step on per-step launches, in lock-step
        if (is_retry(rc) && h->retry_armed && attempt == 0) { h->retry_armed = false; continue; }
        return rc;
    }
    return FSMG_OK;
}

// host lengths of a masked call, checked before any device work: every one in [1, T]
int validate_lengths(fsmg_model* h, const int32_t* len, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (len[i] < 1 || len[i] > h->T)
            return fail(h, FSMG_ERR_INVALID, "length " + std::to_string(len[i]) + " of sequence " + std::to_string(i) + " is outside [1, max_len]");
    return FSMG_OK;
}
// what every masked train entry point checks before it touches the device
int validate_masked_args(fsmg_model* h, const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t on_device) {
    if (!support_len || !query_len) return fail(h, FSMG_ERR_INVALID, "null length pointer");
    int rc = validate_shape(h, N, K, Q);
    if (rc != FSMG_OK || on_device) return rc;
    if ((rc = validate_lengths(h, support_len, (int64_t)N * K)) != FSMG_OK) return rc;
    return validate_lengths(h, query_len, (int64_t)N * Q);
}

// forward + backward + update as ONE captured graph (17 us between two graph launches at cfg-B otherwise)
template <class Stage>
int fused_train_step(fsmg_model* h, int32_t N, int32_t K, int32_t Q, float* loss, Stage&& stage) {
    if (h->comm != nullptr) return dp_train_step(h, loss, [&]() { return forward_backward_core(h, N, K, Q, stage, false); });
    const uint64_t drop_p0 = h->drop_next;
    int rc = forward_backward_core(h, N, K, Q, stage, true);
    if (rc == FSMG_OK) rc = after_update(h, 1.0f, loss);
    if (is_retry(rc) && h->retry_armed) {
        // a persistent step kernel could not get all of its blocks resident (another workload holds the CUs): the
        // update kernels saw the flag and left parameters, Adam state and step counter alone, and the handle has
        // fallen back to one launch per time step -- repeat the step that way
        h->retry_armed = false;
        h->drop_next = drop_p0;             // the repeated pass draws the masks of the pass it repeats
        rc = forward_backward_core(h, N, K, Q, stage, true);
        if (rc == FSMG_OK) rc = after_update(h, 1.0f, loss);
    }
    return rc;
}

// fsmg_forward_backward_state / fsmg_train_step_state behind their argument checks (api_state.hip, which has set state_cur, masked_call and
// the lengths): the R rows as one group, fsmg_*_masked's passes and retries
int state_train_pass(fsmg_model* h, int R, const int32_t* tokens, const int32_t* len, int on_device, bool with_update, float* loss) {
    auto stage = [&]() {
        int r = stage_tokens(h, tokens, 0, tokens, R, on_device);
        if (r == FSMG_OK) r = stage_lengths(h, len, 0, len, R, 0);
        h->state_len = h->d_len;
        return r;
    };
    if (with_update) return fused_train_step(h, 1, 0, R, loss, stage);
    return forward_backward_core(h, 1, 0, R, stage);
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_forward_backward(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K,
                          int32_t Q, int32_t tokens_on_device) {
    if (!h || !support || !query) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);        // the pass orders itself behind a pending update where it first reads the softmax parameters (forward())
    return forward_backward_core(h, N, K, Q, [&]() { return stage_tokens(h, support, N * K, query, N * Q, tokens_on_device); });
}

// ---- device-resident episode table: a split's packed [n_songs][T] token table lives in HBM and an
// episode is an index gather on the GPU (reference src/data/episode.py:62-74, src/data/dataset.py:187-199 fill the same
// rows from the host cache): a step uploads N*(K+Q) indices (180 B at cfg-B) instead of 23 KB of tokens.
int fsmg_upload_table(fsmg_handle h, int32_t table_id, const int32_t* host_table, int64_t n_songs) {
    if (!h || !host_table || table_id < 0 || table_id >= fsmg_model::MAX_TABLES || n_songs <= 0 || n_songs > (1LL << 30) / std::max(1, h->T))
        return h ? fail(h, FSMG_ERR_INVALID, "bad table id / size") : FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->table[table_id]) { hipFree(h->table[table_id]); h->table[table_id] = nullptr; h->table_rows[table_id] = 0; }
    if (h->table_len[table_id]) { hipFree(h->table_len[table_id]); h->table_len[table_id] = nullptr; }      // (the lengths of the table that was here)
    const size_t bytes = sizeof(int) * (size_t)n_songs * h->T;
    if (hipMalloc((void**)&h->table[table_id], bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(token table) failed");
    HIPCK(h, hipMemcpy(h->table[table_id], host_table, bytes, hipMemcpyHostToDevice));
    h->table_rows[table_id] = n_songs;
    return FSMG_OK;
}

int fsmg_upload_table_lengths(fsmg_handle h, int32_t table_id, const int32_t* lengths, int64_t n_songs) {
    if (!h || !lengths || table_id < 0 || table_id >= fsmg_model::MAX_TABLES || n_songs <= 0)
        return h ? fail(h, FSMG_ERR_INVALID, "bad table id / size / null lengths") : FSMG_ERR_INVALID;
    if (!h->table[table_id] || h->table_rows[table_id] != n_songs)
        return fail(h, FSMG_ERR_STATE, "fsmg_upload_table_lengths needs a token table of the same n_songs uploaded under this id first");
    int rc = validate_lengths(h, lengths, n_songs);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->table_len[table_id]) { hipFree(h->table_len[table_id]); h->table_len[table_id] = nullptr; }
    if (hipMalloc((void**)&h->table_len[table_id], sizeof(int) * (size_t)n_songs) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(table lengths) failed");
    HIPCK(h, hipMemcpy(h->table_len[table_id], lengths, sizeof(int) * (size_t)n_songs, hipMemcpyHostToDevice));
    return FSMG_OK;
}

// d_gather / d_gather_len hold an episode of n rows: the MAML table forms' buffers, grown together with the indices'
static int ensure_gather_buffers(fsmg_handle h, int n) {
    if (h->idx_cap >= n && h->gather_cap >= (int64_t)n * h->T) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->d_idx) hipFree(h->d_idx);
    if (h->d_gather) hipFree(h->d_gather);
    if (h->d_gather_len) hipFree(h->d_gather_len);
    h->d_idx = nullptr; h->d_gather = nullptr; h->d_gather_len = nullptr; h->idx_cap = 0; h->gather_cap = 0;
    const int cap = std::max(n, 4096);
    if (hipMalloc((void**)&h->d_idx, sizeof(int) * cap) != hipSuccess || hipMalloc((void**)&h->d_gather, sizeof(int) * (size_t)cap * h->T) != hipSuccess ||
        hipMalloc((void**)&h->d_gather_len, sizeof(int) * cap) != hipSuccess)
        return fail(h, FSMG_ERR_NOMEM, "hipMalloc(episode gather buffers) failed");
    h->idx_cap = cap; h->gather_cap = (int64_t)cap * h->T;
    return FSMG_OK;
}

// The one table gather: the rows sup_idx[0 .. n_sup) then qry_idx[0 .. n_qry) of the table under `table_id`, with_len: and their lengths
// in the same launch (a table without lengths: FSMG_ERR_STATE).  episode: into d_gather / d_gather_len, where the passes of a MAML call
// read them; otherwise into the staging buffers d_tok / d_len of the one pass that is about to run.  An index outside the table raises
// the token-range flag like any bad token.
static int gather_table_rows(fsmg_handle h, int32_t table_id, const int32_t* sup_idx, int n_sup, const int32_t* qry_idx, int n_qry, bool with_len,
                             bool episode) {
    if (table_id < 0 || table_id >= fsmg_model::MAX_TABLES || !h->table[table_id]) return fail(h, FSMG_ERR_STATE, "no token table uploaded under this id");
    if (with_len && !h->table_len[table_id]) return fail(h, FSMG_ERR_STATE, "the table under this id has no lengths (fsmg_upload_table_lengths)");
    const int n = n_sup + n_qry;
    if (episode) {
        const int rc = ensure_gather_buffers(h, n);
        if (rc != FSMG_OK) return rc;
    } else if (h->idx_cap < n) {
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (h->d_idx) hipFree(h->d_idx);
        h->idx_cap = std::max(n, 4096);
        if (hipMalloc((void**)&h->d_idx, sizeof(int) * h->idx_cap) != hipSuccess) { h->idx_cap = 0; h->d_idx = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(indices) failed"); }
    }
    if (n_sup > 0) HIPCK(h, hipMemcpyAsync(h->d_idx, sup_idx, sizeof(int) * n_sup, hipMemcpyHostToDevice, h->stream));
    if (n_qry > 0) HIPCK(h, hipMemcpyAsync(h->d_idx + n_sup, qry_idx, sizeof(int) * n_qry, hipMemcpyHostToDevice, h->stream));
    int32_t* dst = episode ? h->d_gather : h->d_tok;
    if (with_len)
        HIPCK(h, launch_gather_rows_len(h->stream, h->table[table_id], h->table_len[table_id], h->d_idx, n, h->T, (int)h->table_rows[table_id], dst,
                                        episode ? h->d_gather_len : h->d_len, h->d_err));
    else
        HIPCK(h, launch_gather_rows(h->stream, h->table[table_id], h->d_idx, n, h->T, (int)h->table_rows[table_id], dst, h->d_err));
    return FSMG_OK;
}

// a one-pass call's `stage` on the table: a masked call's rows bring their lengths
static int stage_indexed(fsmg_handle h, int32_t table_id, const int32_t* sup_idx, int n_sup, const int32_t* qry_idx, int n_qry) {
    const int rc = gather_table_rows(h, table_id, sup_idx, n_sup, qry_idx, n_qry, h->masked_call, false);
    if (rc != FSMG_OK) return rc;
    if (h->masked_call) h->cur_len = h->d_len;
    h->cur_sup = h->d_tok; h->cur_qry = h->d_tok + (size_t)n_sup * h->T;
    return FSMG_OK;
}

int fsmg_forward_backward_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                  int32_t N, int32_t K, int32_t Q) {
    if (!h || !support_idx || !query_idx) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);        // the pass orders itself behind a pending update where it first reads the softmax parameters (forward())
    return forward_backward_core(h, N, K, Q, [&]() { return stage_indexed(h, table_id, support_idx, N * K, query_idx, N * Q); });
}

int fsmg_train_step_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                            int32_t N, int32_t K, int32_t Q, float* loss) {
    if (!h || !support_idx || !query_idx) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);        // the pass orders itself behind a pending update where it first reads the softmax parameters (forward())
    return fused_train_step(h, N, K, Q, loss, [&]() { return stage_indexed(h, table_id, support_idx, N * K, query_idx, N * Q); });
}

int fsmg_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count) {
    if (!h || !device_ptr || !count) return FSMG_ERR_INVALID;
    *device_ptr = h->G;
    *count = h->n_flat + FSMG_GRAD_TAIL;
    return FSMG_OK;
}

int fsmg_grad_bucket(fsmg_handle h, int32_t bucket, void** device_ptr, int64_t* count) {
    if (!h || !device_ptr || !count || bucket < 0 || bucket >= FSMG_NUM_BUCKETS) return FSMG_ERR_INVALID;
    if (bucket == 0) { *device_ptr = h->G + h->off_w; *count = h->n_flat - h->off_w; }
    else if (bucket == 1) { *device_ptr = h->G; *count = h->off_w; }
    else { *device_ptr = h->G + h->n_flat; *count = FSMG_GRAD_TAIL; }
    return FSMG_OK;
}

int fsmg_stream_wait_bucket(fsmg_handle h, void* stream, int32_t bucket) {
    if (!h || bucket < 0 || bucket >= FSMG_NUM_BUCKETS) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    if (!h->have_grads) return fail(h, FSMG_ERR_STATE, "no backward pass is pending");
    HIPCK(h, hipStreamWaitEvent((hipStream_t)stream, h->ev_bucket[bucket == 0 ? 0 : 1], 0));
    return FSMG_OK;
}

int fsmg_apply_update(fsmg_handle h, float grad_scale, float* loss) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    if (!h->have_grads) return fail(h, FSMG_ERR_STATE, "fsmg_apply_update without a preceding fsmg_forward_backward");
    if (!(grad_scale > 0.f)) return fail(h, FSMG_ERR_INVALID, "grad_scale must be > 0");
    uint32_t bits; std::memcpy(&bits, &grad_scale, 4);
    // a pending Meta-SGD rate gradient: the rates' two launches ride in the update (a graph of its own; fsmg_msgd_enable drops the graphs)
    // (a pending GPhi of the learned optimiser, DESIGN.md 31: one launch, the same way)
    const bool phi = lopt_phi_due(h), rates = msgd_rates_due(h) || phi;
    int rc = run_graphed(h, (phi ? "upl:" : rates ? "upr:" : "up:") + std::to_string(bits) + (h->last_bwd_xcd ? "x" : "s"),
                         [&]() -> int { return apply_update(h, grad_scale, false, rates); });
    h->msgd_pending = false;
    h->lopt_pending = false;
    if (rc != FSMG_OK) return rc;
    return after_update(h, grad_scale, loss);
}

int fsmg_train_step(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                    int32_t tokens_on_device, float* loss) {
    if (!h || !support || !query) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);        // the pass orders itself behind a pending update where it first reads the softmax parameters (forward())
    return fused_train_step(h, N, K, Q, loss, [&]() { return stage_tokens(h, support, N * K, query, N * Q, tokens_on_device); });
}

// ---- padding-masked forms: the same passes with a length per sequence; position t of row b is scored iff t < len[b]
int fsmg_train_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                           int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device, float* loss) {
    if (!h || !support || !query) return FSMG_ERR_INVALID;
    const int rcv = validate_masked_args(h, support_len, query_len, N, K, Q, tokens_on_device);
    if (rcv != FSMG_OK) return rcv;
    BEGIN_CALL(h, true);
    begin_masked(h, N * (K + Q), 1);
    return fused_train_step(h, N, K, Q, loss, [&]() {
        const int r = stage_tokens(h, support, N * K, query, N * Q, tokens_on_device);
        return r != FSMG_OK ? r : stage_lengths(h, support_len, N * K, query_len, N * Q, tokens_on_device);
    });
}

int fsmg_forward_backward_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                                 int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device) {
    if (!h || !support || !query) return FSMG_ERR_INVALID;
    const int rcv = validate_masked_args(h, support_len, query_len, N, K, Q, tokens_on_device);
    if (rcv != FSMG_OK) return rcv;
    BEGIN_CALL(h, true);
    begin_masked(h, N * (K + Q), 1);
    return forward_backward_core(h, N, K, Q, [&]() {
        const int r = stage_tokens(h, support, N * K, query, N * Q, tokens_on_device);
        return r != FSMG_OK ? r : stage_lengths(h, support_len, N * K, query_len, N * Q, tokens_on_device);
    });
}

int fsmg_train_step_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                   int32_t N, int32_t K, int32_t Q, float* loss) {
    if (!h || !support_idx || !query_idx) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);
    begin_masked(h, N * (K + Q), 1);
    return fused_train_step(h, N, K, Q, loss, [&]() { return stage_indexed(h, table_id, support_idx, N * K, query_idx, N * Q); });
}

int fsmg_forward_backward_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                         int32_t N, int32_t K, int32_t Q) {
    if (!h || !support_idx || !query_idx) return FSMG_ERR_INVALID;
    BEGIN_CALL(h, true);
    begin_masked(h, N * (K + Q), 1);
    return forward_backward_core(h, N, K, Q, [&]() { return stage_indexed(h, table_id, support_idx, N * K, query_idx, N * Q); });
}

static int eval_batch_core(fsmg_handle h, const int32_t* queries, const int32_t* query_len, int32_t n_episodes, int32_t N, int32_t Q,
                           int32_t tokens_on_device, float* nll, bool masked, bool repeat_chunk = true);

}  // extern "C"

// ---- cfg-E (BASELINE.json configs[4]): MAML-style inner / outer loop, first order.  DESIGN.md "cfg-E", 22 (per-song lengths), 28 (the drivers).
namespace fsmg_host {

// The prologue is fsmg_forward_backward's, and it is the pass's own: a pass repeated after an update (step_with_update) orders itself
// behind that update's pending half here.  The flag is set behind the prologue, which clears it, and the pass's own `stage` stages its
// lengths (a repeat restages them); what runs next at theta' (the update, a decode) is not a masked pass.
int rows_pass(fsmg_model* h, const int32_t* rows, const int32_t* len, int32_t N, int32_t R, int32_t on_device) {
    BEGIN_CALL(h, true);
    if (len) begin_masked(h, N * R, 1);
    const int rc = forward_backward_core(h, N, R, 0, [&]() {
        const int r = stage_tokens(h, rows, N * R, rows, 0, on_device);
        return r != FSMG_OK || !len ? r : stage_lengths(h, len, N * R, len, 0, on_device);
    });
    h->masked_call = false;
    return rc;
}

// the window [lo, hi) is written to its fixed address in stream order before the pass, outside any capture, so a replayed graph reads
// the window of THIS call (dynamic evaluation)
int window_rows_pass(fsmg_model* h, const int32_t* rows, const int32_t* len, int32_t n, int lo, int hi) {
    BEGIN_CALL(h, true);
    begin_masked(h, n, 1);
    h->window_call = true;
    const bool suppress0 = h->drop_suppress;
    h->drop_suppress = true;                    // dynamic evaluation is never dropped
    const int rc = forward_backward_core(h, 1, n, 0, [&]() {
        int r = stage_tokens(h, rows, n, rows, 0, 0);
        if (r == FSMG_OK) r = stage_lengths(h, len, n, len, 0, 0);
        if (r == FSMG_OK) HIPCK(h, launch_set_window(h->stream, h->d_win, lo, hi));
        return r;
    });
    h->drop_suppress = suppress0;
    h->masked_call = false;
    h->window_call = false;
    return rc;
}

// with Meta-SGD enabled the adaptation of a train form starts S from zero and collects every applied step
int maml_adapt(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, bool train) {
    int rc = save_theta(h);
    if (rc == FSMG_OK && h->msgd_on && train) rc = msgd_begin_sum(h);
    if (rc == FSMG_OK && h->lopt_on) rc = lopt_begin(h, train);         // the learned optimiser: the gates restart
    const bool suppress0 = h->drop_suppress;
    if (!train) h->drop_suppress = true;        // the adaptation of an eval / decode / score form is never dropped
    for (int i = 0; rc == FSMG_OK && i < inner_steps; ++i) {
        rc = rows_pass(h, e.sup, e.masked ? e.slen : nullptr, e.N, e.K, e.on_device);       // support rows only
        if (rc == FSMG_OK) rc = h->lopt_on ? lopt_inner_update(h, inner_lr) : h->msgd_on ? msgd_inner_update(h, inner_lr, train) : sgd_update(h, inner_lr);
    }
    h->drop_suppress = suppress0;
    return rc;
}

int adapt_flag(fsmg_model* h) {
    int err = 0;
    HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!err) return FSMG_OK;
    HIPCK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));
    if (err == 2) on_timeout(h);
    else if (err == 4) on_softmax_range(h);
    return report(h, err);
}

// (theta was never saved where save_theta's first allocation failed: nothing to keep or to put back.  Neither copy reads the two flags.)
int end_adaptation(fsmg_model* h) {
    h->masked_call = false; h->window_call = false;
    const int rc_keep = h->P_saved ? keep_theta_prime(h) : FSMG_OK;
    const int rc = h->P_saved ? restore_theta(h) : FSMG_OK;        // theta comes back whatever happened
    h->have_grads = false;
    return rc != FSMG_OK ? rc : rc_keep;
}

int at_adapted_theta(fsmg_model* h, const std::function<int()>& adapt, const std::function<int()>& body) {
    int rc = FSMG_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
        rc = adapt();
        if (rc == FSMG_OK) rc = body();
        const int rc_end = end_adaptation(h);
        if (rc == FSMG_OK) rc = rc_end;
        if (!(is_retry(rc) && h->retry_armed)) break;
        h->retry_armed = false;                        // adapted with garbage (skipped) steps: repeat on per-step launches
    }
    return rc;
}

int step_with_update(fsmg_model* h, float* loss, const std::function<int()>& forward_backward) {
    if (h->comm != nullptr) return dp_train_step(h, loss, forward_backward);      // the gradient exchanged like a plain step's (1 / world takes the mean)
    const uint64_t drop_p0 = h->drop_next;
    int rc = forward_backward();
    if (rc != FSMG_OK) return rc;
    rc = fsmg_apply_update(h, 1.0f, loss);
    if (is_retry(rc) && h->retry_armed) {        // same recovery as fsmg_train_step: nothing was updated, repeat per step
        h->retry_armed = false;
        h->drop_next = drop_p0;                  // the repeated passes draw the masks of the passes they repeat
        rc = forward_backward();
        if (rc == FSMG_OK) rc = fsmg_apply_update(h, 1.0f, loss);
    }
    return rc;
}

int gather_episode(fsmg_model* h, int32_t table_id, bool with_len, const int32_t* support_idx, const int32_t* query_idx, int32_t N, int32_t K,
                   int32_t Q, Episode* e) {
    const int rc = gather_table_rows(h, table_id, support_idx, N * K, query_idx, N * Q, with_len, true);
    if (rc != FSMG_OK) return rc;
    *e = token_episode(h->d_gather, h->d_gather + (size_t)N * K * h->T, with_len ? h->d_gather_len : nullptr,
                       with_len ? h->d_gather_len + (size_t)N * K : nullptr, N, K, Q, 1);
    return FSMG_OK;
}

int locate_episode(fsmg_model* h, int32_t table_id, bool with_len, const int32_t* support, const int32_t* query, const int32_t* support_len,
                   const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int on_device, Episode* e) {
    if (table_id >= 0) return gather_episode(h, table_id, with_len, support, query, N, K, Q, e);
    *e = token_episode(support, query, support_len, query_len, N, K, Q, on_device);
    return FSMG_OK;
}

// The prologue is the call's own: a repeat behind an update (step_with_update, dp_train_step) settles that update's pending half
// before theta is saved.  The gradient of the query pass at theta' stays pending; theta comes back under it.
int maml_forward_backward(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr) {
    int rc = lopt_check_train(h, inner_steps);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    rc = maml_adapt(h, e, inner_steps, inner_lr, true);
    if (rc == FSMG_OK) rc = rows_pass(h, e.qry, e.masked ? e.qlen : nullptr, e.N, e.Q, e.on_device);       // query rows at theta'
    if (rc == FSMG_OK && h->msgd_on) rc = msgd_rate_gradient(h);
    if (rc == FSMG_OK && h->lopt_on) rc = lopt_meta_gradient(h, true, 1.0);
    const bool pending = h->have_grads;
    const int rc_end = end_adaptation(h);
    h->have_grads = pending;
    return rc != FSMG_OK ? rc : rc_end;
}

int maml_step(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, float* loss) {
    // per-rank inner loop (no communication); a repeat carries the lengths like the first attempt
    return step_with_update(h, loss, [&]() { return maml_forward_backward(h, e, inner_steps, inner_lr); });
}

int maml_eval(fsmg_model* h, const Episode& e, int32_t inner_steps, float inner_lr, float* nll) {
    BEGIN_CALL(h);
    // The flag of a time-out / token error inside the adaptation is still set: the query pass reads and reports it (reading it here
    // would be one more synchronisation per call).  The query pass must not repeat its chunk on its own as fsmg_eval_step does: the
    // inner updates of a timed-out adaptation were skipped, the repeated chunk would succeed at the UNADAPTED theta and its NLL would
    // be returned as if nothing had happened -- the adaptation is repeated with it, lengths and all.
    return at_adapted_theta(
        h, [&]() { return maml_adapt(h, e, inner_steps, inner_lr, false); },
        [&]() { return eval_batch_core(h, e.qry, e.masked ? e.qlen : nullptr, 1, e.N, e.Q, e.on_device, nll, e.masked, false); });
}

// One repeat on per-step launches when the adaptation ran garbage (skipped) steps: the error word is read before the body, because the
// body (a decode, a scoring pass) would run at a theta' that is not one.
int with_adapted_theta(fsmg_model* h, const int32_t* support, int32_t n_support_rows, int32_t inner_steps, float inner_lr,
                       int32_t support_on_device, const std::function<int()>& at_theta_prime, const int32_t* support_len, bool masked) {
    if (masked && !support_len) return fail(h, FSMG_ERR_INVALID, "null length pointer");
    if (!support || n_support_rows <= 0 || inner_steps < 0 || inner_steps > 64 || !(inner_lr >= 0.f) || !std::isfinite(inner_lr) ||
        (support_on_device != 0 && support_on_device != 1))
        return fail(h, FSMG_ERR_INVALID, "bad support / n_support_rows / inner_steps / inner_lr");
    if (masked) {         // host lengths before any device work; device lengths meet the range check of the kernel that builds the weights
        int rcv = validate_shape(h, 1, n_support_rows, 0);
        if (rcv == FSMG_OK && !support_on_device) rcv = validate_lengths(h, support_len, n_support_rows);
        if (rcv != FSMG_OK) return rcv;
    }
    BEGIN_CALL(h);
    const Episode e = token_episode(support, nullptr, masked ? support_len : nullptr, nullptr, 1, n_support_rows, 0, support_on_device);
    return at_adapted_theta(
        h,
        [&]() {
            const int rc = maml_adapt(h, e, inner_steps, inner_lr, false);
            return rc != FSMG_OK ? rc : adapt_flag(h);           // a time-out / token error inside the adaptation: theta' is not usable
        },
        at_theta_prime);
}

}  // namespace fsmg_host

extern "C" {

static int check_inner_loop(fsmg_handle h, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr) {
    if (inner_steps < 0 || inner_steps > 64 || !(inner_lr >= 0.f) || K <= 0 || Q <= 0) return fail(h, FSMG_ERR_INVALID, "bad inner_steps / inner_lr / K / Q");
    return FSMG_OK;
}

int fsmg_maml_forward_backward(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                               int32_t inner_steps, float inner_lr, int32_t tokens_on_device) {
    if (!h || !support || !query) return FSMG_ERR_INVALID;
    const int rcv = check_inner_loop(h, K, Q, inner_steps, inner_lr);
    if (rcv != FSMG_OK) return rcv;
    return maml_forward_backward(h, token_episode(support, query, nullptr, nullptr, N, K, Q, tokens_on_device), inner_steps, inner_lr);
}

int fsmg_maml_step(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                   int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* loss) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    if (!support || !query) return FSMG_ERR_INVALID;
    const int rcv = check_inner_loop(h, K, Q, inner_steps, inner_lr);
    if (rcv != FSMG_OK) return rcv;
    return maml_step(h, token_episode(support, query, nullptr, nullptr, N, K, Q, tokens_on_device), inner_steps, inner_lr, loss);
}

int fsmg_maml_eval(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                   int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* nll) {
    if (!h || !support || !query || !nll) return FSMG_ERR_INVALID;
    const int rcv = check_inner_loop(h, K, Q, inner_steps, inner_lr);
    if (rcv != FSMG_OK) return rcv;
    return maml_eval(h, token_episode(support, query, nullptr, nullptr, N, K, Q, tokens_on_device), inner_steps, inner_lr, nll);
}

// ---- cfg-E with per-song lengths: every inner step over the support rows' valid positions, the outer pass over the query rows'
static int validate_maml_masked_args(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                                     int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, int32_t on_device) {
    if (!support || !query) return fail(h, FSMG_ERR_INVALID, "null token pointer");
    const int rc = check_inner_loop(h, K, Q, inner_steps, inner_lr);
    return rc != FSMG_OK ? rc : validate_masked_args(h, support_len, query_len, N, K, Q, on_device);
}

int fsmg_maml_forward_backward_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                                      int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, int32_t tokens_on_device) {
    if (!h) return FSMG_ERR_INVALID;
    const int rcv = validate_maml_masked_args(h, support, query, support_len, query_len, N, K, Q, inner_steps, inner_lr, tokens_on_device);
    if (rcv != FSMG_OK) return rcv;
    return maml_forward_backward(h, token_episode(support, query, support_len, query_len, N, K, Q, tokens_on_device), inner_steps, inner_lr);
}

int fsmg_maml_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                          int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* loss) {
    if (!h) return FSMG_ERR_INVALID;
    const int rcv = validate_maml_masked_args(h, support, query, support_len, query_len, N, K, Q, inner_steps, inner_lr, tokens_on_device);
    if (rcv != FSMG_OK) return rcv;
    BEGIN_CALL(h);
    return maml_step(h, token_episode(support, query, support_len, query_len, N, K, Q, tokens_on_device), inner_steps, inner_lr, loss);
}

int fsmg_maml_eval_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len, const int32_t* query_len,
                          int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* nll) {
    if (!h || !nll) return FSMG_ERR_INVALID;
    const int rcv = validate_maml_masked_args(h, support, query, support_len, query_len, N, K, Q, inner_steps, inner_lr, tokens_on_device);
    if (rcv != FSMG_OK) return rcv;
    return maml_eval(h, token_episode(support, query, support_len, query_len, N, K, Q, tokens_on_device), inner_steps, inner_lr, nll);
}

// cfg-E on the device-resident split table, behind the entry point's null checks: the gather (gather_episode), then what the token
// form of the same call checks -- in the masked forms the lengths come out of the same gather and reach the passes as device lengths
static int indexed_episode(fsmg_handle h, int32_t table_id, bool masked, const int32_t* support_idx, const int32_t* query_idx, int32_t N, int32_t K,
                           int32_t Q, int32_t inner_steps, float inner_lr, Episode* e) {
    BEGIN_CALL(h);
    int rc = gather_episode(h, table_id, masked, support_idx, query_idx, N, K, Q, e);
    if (rc == FSMG_OK) rc = check_inner_loop(h, K, Q, inner_steps, inner_lr);
    if (rc == FSMG_OK && masked) rc = validate_masked_args(h, e->slen, e->qlen, N, K, Q, 1);
    return rc;
}

int fsmg_maml_forward_backward_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                       int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr) {
    if (!h || !support_idx || !query_idx || N <= 0 || K <= 0 || Q <= 0) return FSMG_ERR_INVALID;
    Episode e;
    const int rc = indexed_episode(h, table_id, false, support_idx, query_idx, N, K, Q, inner_steps, inner_lr, &e);
    return rc != FSMG_OK ? rc : maml_forward_backward(h, e, inner_steps, inner_lr);
}

int fsmg_maml_step_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                           int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, float* loss) {
    if (!h || !support_idx || !query_idx || N <= 0 || K <= 0 || Q <= 0) return FSMG_ERR_INVALID;
    Episode e;
    const int rc = indexed_episode(h, table_id, false, support_idx, query_idx, N, K, Q, inner_steps, inner_lr, &e);
    return rc != FSMG_OK ? rc : maml_step(h, e, inner_steps, inner_lr, loss);
}

int fsmg_maml_forward_backward_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                              int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr) {
    if (!h || !support_idx || !query_idx || N <= 0 || K <= 0 || Q <= 0) return FSMG_ERR_INVALID;
    Episode e;
    const int rc = indexed_episode(h, table_id, true, support_idx, query_idx, N, K, Q, inner_steps, inner_lr, &e);
    return rc != FSMG_OK ? rc : maml_forward_backward(h, e, inner_steps, inner_lr);
}

int fsmg_maml_step_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                  int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, float* loss) {
    if (!h || !support_idx || !query_idx || N <= 0 || K <= 0 || Q <= 0) return FSMG_ERR_INVALID;
    Episode e;
    const int rc = indexed_episode(h, table_id, true, support_idx, query_idx, N, K, Q, inner_steps, inner_lr, &e);
    return rc != FSMG_OK ? rc : maml_step(h, e, inner_steps, inner_lr, loss);
}

}  // extern "C"

extern "C" {

// query_len != nullptr: the padding-masked form -- each episode's NLL over its own n_valid
// repeat_chunk: a chunk whose persistent kernel timed out is repeated here on per-step launches (false: the caller repeats -- fsmg_maml_eval,
// whose adaptation has to be repeated with it)
static int eval_batch_core(fsmg_handle h, const int32_t* queries, const int32_t* query_len, int32_t n_episodes, int32_t N, int32_t Q,
                           int32_t tokens_on_device, float* nll, bool masked, bool repeat_chunk) {
    if (!h || !queries || !nll || n_episodes <= 0) return FSMG_ERR_INVALID;
    int rc = validate_shape(h, N, 0, Q);
    if (rc != FSMG_OK) return rc;
    const int per = N * Q;
    if (per <= 0) return fail(h, FSMG_ERR_INVALID, "empty query set");
    if (masked) {
        if (!query_len) return fail(h, FSMG_ERR_INVALID, "null length pointer");
        if ((int64_t)n_episodes * per > (1LL << 30)) return fail(h, FSMG_ERR_INVALID, "too many query rows");
        if (!tokens_on_device && (rc = validate_lengths(h, query_len, (int64_t)n_episodes * per)) != FSMG_OK) return rc;
    }
    BEGIN_CALL(h);
    // validation episodes are independent: batch up to EVAL_EPISODES of them per pass so that the recurrent
    // chain (one launch per time step regardless of the row count) is amortised over many rows
    constexpr int EVAL_EPISODES = 16;
    if ((rc = ensure_scratch(h, per * std::min<int>(n_episodes, EVAL_EPISODES))) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    const int chunk_eps = std::min<int>(h->Bcap / per, 64);
    if (h->eval_cap < chunk_eps) {
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (h->d_eval) hipFree(h->d_eval);
        HIPCK(h, hipMalloc((void**)&h->d_eval, sizeof(float) * chunk_eps));
        h->eval_cap = chunk_eps;
    }
    bool retried = false;
    for (int e0 = 0; e0 < n_episodes; e0 += chunk_eps) {
        const int ne = std::min(chunk_eps, n_episodes - e0);
        const int B = ne * per;
        choose_schedule(h, B);
        if (pass_reads_cs(h, B, false) && (rc = ensure_cs(h)) != FSMG_OK) return rc;
        const int32_t* q = queries + (size_t)e0 * per * h->T;
        if ((rc = stage_tokens(h, q, 0, q, B, tokens_on_device)) != FSMG_OK) return rc;
        if (masked) {
            begin_masked(h, per, ne);
            if ((rc = stage_lengths(h, query_len, 0, query_len + (size_t)e0 * per, B, tokens_on_device)) != FSMG_OK) return rc;
        }
        rc = run_graphed(h, (masked ? "evm:" : "ev:") + std::to_string(per) + ":" + std::to_string(ne), [&]() -> int {
            int r = token_prep(h, 0, B);
            if (r == FSMG_OK) r = forward(h, B, per, ne, h->d_eval, false);
            return r;
        });
        if (rc != FSMG_OK) return rc;
        h->lastB = B;
        rc = check_tokens_and_read(h, h->d_eval, 1.0f, nll + e0, ne);
        if (repeat_chunk && is_retry(rc) && h->retry_armed && !retried) {
            // a persistent kernel could not get its blocks resident: the handle has switched to one launch per time
            // step; repeat this chunk that way (validation must not abort a training run, nor leave peer ranks hanging)
            h->retry_armed = false;
            retried = true;
            e0 -= chunk_eps;
            continue;
        }
        if (rc != FSMG_OK) return rc;
        retried = false;
    }
    return FSMG_OK;
}

int fsmg_eval_batch(fsmg_handle h, const int32_t* queries, int32_t n_episodes, int32_t N, int32_t Q,
                    int32_t tokens_on_device, float* nll) {
    return eval_batch_core(h, queries, nullptr, n_episodes, N, Q, tokens_on_device, nll, false);
}

int fsmg_eval_step(fsmg_handle h, const int32_t* query, int32_t N, int32_t Q, int32_t tokens_on_device, float* nll) {
    return fsmg_eval_batch(h, query, 1, N, Q, tokens_on_device, nll);
}

int fsmg_eval_batch_masked(fsmg_handle h, const int32_t* queries, const int32_t* query_len, int32_t n_episodes, int32_t N, int32_t Q,
                           int32_t tokens_on_device, float* nll) {
    return eval_batch_core(h, queries, query_len, n_episodes, N, Q, tokens_on_device, nll, true);
}

int fsmg_eval_step_masked(fsmg_handle h, const int32_t* query, const int32_t* query_len, int32_t N, int32_t Q, int32_t tokens_on_device, float* nll) {
    return fsmg_eval_batch_masked(h, query, query_len, 1, N, Q, tokens_on_device, nll);
}

}  // extern "C"
