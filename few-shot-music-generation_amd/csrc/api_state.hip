// Batched passes from a carried LSTM state: fsmg_score_state, fsmg_eval_step_state, fsmg_forward_backward_state,
// fsmg_train_step_state -- truncated BPTT over segments of max_len tokens, scoring and evaluation under full context.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in state.hip.
// A state pass is a padding-masked pass of ONE group of R = state rows with three differences, each a hook on fsmg_model::state_cur:
// slot 0 of every layer is the state's h, c instead of a zero fill (state_import, from forward()), position 0 reads the state's pending
// token instead of the start word (state_token_prep, from token_prep()), and the state takes slot len[b] and the segment's tokens when
// the pass is over (state_export).  It runs the serial order (choose_schedule); inside it every kernel choice is the handle's.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

int state_token_prep(fsmg_model* h, int B, bool table) {
    const fsmg_dstate_s* st = h->state_cur;
    HIPCK(h, launch_state_weights(h->stream, h->state_len, B, h->T, h->roww, h->d_nvalid));
    HIPCK(h, launch_state_token_prep(h->stream, h->cur_qry, B, h->T, h->V, h->V, h->state_len, st->ctx, st->history + 1, st->kept(), h->X, h->Y,
                                     h->d_err, table ? h->tok_first : nullptr, table ? h->tok_count : nullptr));
    return FSMG_OK;
}

// which hand-off copy layer l's chain reads at index 0 follows the same tests forward() chooses the chain by
int state_import(fsmg_model* h, int l, int B, bool xcd) {
    const fsmg_dstate_s* st = h->state_cur;
    const int Hp = h->Hp;
    StateImportArgs a{};
    a.h = st->h + (size_t)l * st->R * Hp; a.c = st->c + (size_t)l * st->R * Hp;
    a.Hs0 = h->Hs[l]; a.Cs0 = h->Cs[l]; a.B = B; a.Hp = Hp;
    if (!xcd) {
        a.kind = STATE_HAND_HF; a.hand = h->HF[l];
    } else {
        const bool bf16 = h->xcd_bx3 && Hp != 256;
        const long long step_f = lstm_xcd_hx_floats(B, 0, Hp, h->xcd_bx3, 0);       // one time index of the layout the launch is instantiated for
        a.kind = bf16 ? STATE_HAND_HX16 : STATE_HAND_HX32; a.hand = h->HX;
        a.ng = Hp == 1024 ? 4 : (Hp == 512 ? 8 : 16);
        a.nq = bf16 ? Hp / 128 : Hp / 256;
        const long long per_row = bf16 ? (long long)a.ng * a.nq * 192 : (long long)a.ng * a.nq * 256;
        a.rows = (int)(step_f / per_row);
        if ((Hp != 256 && Hp != 512 && Hp != 1024) || step_f <= 0 || step_f % per_row != 0 || a.rows < 4 || a.rows > 16 || (a.rows & 3) != 0 ||
            step_f > h->hx_floats || (long long)a.ng * a.rows < B)
            return fail(h, FSMG_ERR_STATE, "internal: no hand-off layout for a state import at this shape");
    }
    ScopedTimer tm(h, "state_import");
    HIPCK(h, launch_state_import(h->stream, a));
    ++h->n_state_imports[a.kind];
    return FSMG_OK;
}

int state_export(fsmg_model* h, int B) {
    fsmg_dstate_s* st = h->state_cur;
    const int Hp = h->Hp;
    ScopedTimer tm(h, "state_export");
    for (int l = 0; l < h->L; ++l)
        HIPCK(h, launch_state_export(h->stream, h->Hs[l], h->Cs[l], B, Hp, h->T, h->state_len, st->h + (size_t)l * st->R * Hp,
                                     st->c + (size_t)l * st->R * Hp, h->d_err));
    const int keep = (int)std::min<long long>(st->n_ctx + h->T, st->history);
    HIPCK(h, launch_state_export_ctx(h->stream, h->cur_qry, B, h->T, h->V, h->state_len, st->ctx, st->history + 1, st->kept(), keep, h->d_err));
    return FSMG_OK;
}

namespace {

// the call's state pass is over, however it ended
struct StateScope {
    fsmg_model* h;
    ~StateScope() { h->state_cur = nullptr; h->state_len = nullptr; h->masked_call = false; }
};

// what every state entry point refuses before any device work; *len_out = the lengths the pass runs with (NULL lengths: all T)
int check_state_args(fsmg_model* h, fsmg_dstate st, const int32_t* tokens, const int32_t* lengths, int32_t on_device, fsmg_dstate_s** st_out,
                     std::vector<int32_t>* len_out) {
    fsmg_dstate_s* s = nullptr;
    for (fsmg_dstate_s* q : h->dstates)
        if (q == st && st != nullptr) s = q;
    if (!s) return fail(h, FSMG_ERR_INVALID, "not a decode state of this handle (never created here, or already destroyed)");
    if (!tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    if (on_device != 0 && on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (s->R > FSMG_STATE_PASS_ROWS) return fail(h, FSMG_ERR_INVALID, "the state has more rows than one pass takes (FSMG_STATE_PASS_ROWS)");
    len_out->assign((size_t)s->R, h->T);
    if (lengths) {
        bool any = false;
        for (int r = 0; r < s->R; ++r) {
            if (lengths[r] < 0 || lengths[r] > h->T) return fail(h, FSMG_ERR_INVALID, "every length must be in [0, max_len]");
            (*len_out)[(size_t)r] = lengths[r];
            any = any || lengths[r] > 0;
        }
        if (!any) return fail(h, FSMG_ERR_INVALID, "every length is 0: the pass would score nothing");
    }
    if (s->n_ctx > (1LL << 62) - h->T) return fail(h, FSMG_ERR_INVALID, "the state's context count would overflow");
    if (!on_device) {
        const int rc = check_host_tokens(h, tokens, (size_t)s->R * h->T);
        if (rc != FSMG_OK) return rc;
    }
    *st_out = s;
    return FSMG_OK;
}

// the pass begins: behind BEGIN_CALL, which clears these
void begin_state(fsmg_model* h, fsmg_dstate_s* st) {
    h->state_cur = st; h->state_len = h->d_len;
    begin_masked(h, st->R, 1);
}

// a forward-only state pass over the state's R rows: launch() enqueues it (token_prep, forward, what reads the result) and read_back()
// the copies to the host; the error word comes back behind them.  run_passes' contract for one pass: a time-out repeats it once on
// per-step launches -- the export saw the flag and left the state alone, so the repeat imports what this pass imported.
int forward_state_pass(fsmg_model* h, fsmg_dstate_s* st, const int32_t* tokens, const std::vector<int32_t>& len, int on_device,
                       const std::function<int(int)>& launch, const std::function<int(int)>& read_back) {
    const int B = st->R;
    int rc;
    if ((rc = ensure_scratch(h, B)) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    for (int attempt = 0; attempt < 2; ++attempt) {
        begin_state(h, st);
        choose_schedule(h, B);
        if (pass_reads_cs(h, B, false) && (rc = ensure_cs(h)) != FSMG_OK) return rc;
        if ((rc = stage_tokens(h, tokens, 0, tokens, B, on_device)) != FSMG_OK) return rc;
        if ((rc = stage_lengths(h, len.data(), 0, len.data(), B, 0)) != FSMG_OK) return rc;
        h->state_len = h->d_len;
        if ((rc = launch(B)) != FSMG_OK) return rc;
        if ((rc = state_export(h, B)) != FSMG_OK) return rc;
        h->lastB = B;
        if ((rc = read_back(B)) != FSMG_OK) return rc;
        int err = 0;
        HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (!err) { st->n_ctx += h->T; return FSMG_OK; }
        HIPCK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));
        if (err == 2) on_timeout(h);
        rc = report(h, err);
        if (!is_retry(rc) || !h->retry_armed || attempt == 1) return rc;
        h->retry_armed = false;
    }
    return FSMG_OK;
}

}  // namespace
}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_score_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths,
                     float* out_logprob, int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_config_header(h, c, "fsmg_state_config", FSMG_STATE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (!out_logprob && !out_rank && !out_entropy && !out_argmax && !out_row_nll) return fail(h, FSMG_ERR_INVALID, "every output is null");
    fsmg_dstate_s* s = nullptr;
    std::vector<int32_t> len;
    if ((rc = check_state_args(h, st, tokens, lengths, c->tokens_on_device, &s, &len)) != FSMG_OK) return rc;
    BEGIN_CALL(h);
    StateScope scope{h};
    const int R = s->R, T = h->T;
    std::vector<float> lp_own;
    float* lp_host = out_logprob;
    if (out_row_nll && !lp_host) { lp_own.resize((size_t)R * T); lp_host = lp_own.data(); }
    const int mask = (lp_host ? 1 : 0) | (out_rank ? 2 : 0) | (out_entropy ? 4 : 0) | (out_argmax ? 8 : 0);
    auto d_out = [&](int B, int k) { return h->score_out + (size_t)k * B * T; };      // fsmg_score's device outputs
    rc = forward_state_pass(
        h, s, tokens, len, c->tokens_on_device,
        [&](int B) -> int {
            int r = token_prep(h, 0, B);
            if (r == FSMG_OK) r = forward(h, B, B, 1, nullptr, false, HEAD_LOGITS);
            if (r != FSMG_OK) return r;
            ScopedTimer tm(h, "ce");
            HIPCK(h, launch_score_rows(h->stream, h->logits, h->V1p, B * T, h->V1, h->Y, B, T, (mask & 1) ? d_out(B, 0) : nullptr,
                                       (mask & 2) ? (int*)d_out(B, 2) : nullptr, (mask & 4) ? d_out(B, 1) : nullptr,
                                       (mask & 8) ? (int*)d_out(B, 3) : nullptr));
            return FSMG_OK;
        },
        [&](int B) -> int {
            const size_t bytes = sizeof(float) * (size_t)B * T;
            if (mask & 1) HIPCK(h, hipMemcpyAsync(lp_host, d_out(B, 0), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 2) HIPCK(h, hipMemcpyAsync(out_rank, d_out(B, 2), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 4) HIPCK(h, hipMemcpyAsync(out_entropy, d_out(B, 1), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 8) HIPCK(h, hipMemcpyAsync(out_argmax, d_out(B, 3), bytes, hipMemcpyDeviceToHost, h->stream));
            return FSMG_OK;
        });
    if (rc != FSMG_OK) return rc;
    for (int r = 0; r < R; ++r)             // fsmg_score_masked's outputs: 0 behind a row's end
        for (size_t i = (size_t)r * T + len[(size_t)r]; i < (size_t)(r + 1) * T; ++i) {
            if (mask & 1) lp_host[i] = 0.0f;
            if (mask & 2) out_rank[i] = 0;
            if (mask & 4) out_entropy[i] = 0.0f;
            if (mask & 8) out_argmax[i] = 0;
        }
    if (out_row_nll) row_nll_masked(lp_host, R, T, 0, 0, len.data(), out_row_nll);
    return FSMG_OK;
}

int fsmg_eval_step_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths,
                         float* nll, int32_t* n_valid) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_config_header(h, c, "fsmg_state_config", FSMG_STATE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (!nll) return fail(h, FSMG_ERR_INVALID, "null nll");
    fsmg_dstate_s* s = nullptr;
    std::vector<int32_t> len;
    if ((rc = check_state_args(h, st, tokens, lengths, c->tokens_on_device, &s, &len)) != FSMG_OK) return rc;
    BEGIN_CALL(h);
    StateScope scope{h};
    if (h->eval_cap < 1) {
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (h->d_eval) hipFree(h->d_eval);
        h->d_eval = nullptr;
        if (hipMalloc((void**)&h->d_eval, sizeof(float) * 64) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(eval NLLs) failed");
        h->eval_cap = 64;
    }
    float out = 0.f;
    rc = forward_state_pass(
        h, s, tokens, len, c->tokens_on_device,
        [&](int B) -> int {
            int r = token_prep(h, 0, B);
            if (r == FSMG_OK) r = forward(h, B, B, 1, h->d_eval, false);
            return r;
        },
        [&](int) -> int {
            HIPCK(h, hipMemcpyAsync(&out, h->d_eval, sizeof(float), hipMemcpyDeviceToHost, h->stream));
            return FSMG_OK;
        });
    if (rc != FSMG_OK) return rc;
    *nll = out;
    if (n_valid) { long long nv = 0; for (int32_t l : len) nv += l; *n_valid = (int32_t)nv; }
    return FSMG_OK;
}

int fsmg_forward_backward_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_config_header(h, c, "fsmg_state_config", FSMG_STATE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    fsmg_dstate_s* s = nullptr;
    std::vector<int32_t> len;
    if ((rc = check_state_args(h, st, tokens, lengths, c->tokens_on_device, &s, &len)) != FSMG_OK) return rc;
    if (h->comm != nullptr)
        return fail(h, FSMG_ERR_STATE, "a state pass on a handle with a library communicator: a step a peer skips would leave this rank's state advanced");
    BEGIN_CALL(h, true);
    StateScope scope{h};
    begin_state(h, s);
    rc = state_train_pass(h, s->R, tokens, len.data(), c->tokens_on_device, false, nullptr);
    if (rc != FSMG_OK) return rc;
    // whether the state advanced is decided on the device (the export looks at the error word, which stays up for fsmg_apply_update to
    // report): the host's counter follows it
    int err = 0;
    HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!err) s->n_ctx += h->T;
    return FSMG_OK;
}

int fsmg_train_step_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths, float* loss) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_config_header(h, c, "fsmg_state_config", FSMG_STATE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (!loss) return fail(h, FSMG_ERR_INVALID, "null loss: the call reads it back to learn whether the step (and the state) went through");
    fsmg_dstate_s* s = nullptr;
    std::vector<int32_t> len;
    if ((rc = check_state_args(h, st, tokens, lengths, c->tokens_on_device, &s, &len)) != FSMG_OK) return rc;
    if (h->comm != nullptr)
        return fail(h, FSMG_ERR_STATE, "a state pass on a handle with a library communicator: a step a peer skips would leave this rank's state advanced");
    BEGIN_CALL(h, true);
    StateScope scope{h};
    begin_state(h, s);
    rc = state_train_pass(h, s->R, tokens, len.data(), c->tokens_on_device, true, loss);
    if (rc == FSMG_OK) s->n_ctx += h->T;
    return rc;
}

}  // extern "C"
