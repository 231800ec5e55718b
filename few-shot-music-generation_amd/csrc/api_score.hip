// Scoring of given songs: fsmg_score and fsmg_maml_score (at theta', through with_adapted_theta in api_step.hip).
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernel lives in score.hip.  DESIGN.md 15.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

namespace {

int check_score_config(fsmg_model* h, const fsmg_score_config* c, const int32_t* tokens, const void* const outs[5]) {
    const int rc = check_config_header(h, c, "fsmg_score_config", FSMG_SCORE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (c->n_rows < 1 || c->n_rows > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n_rows must be in [1, 2^20]");
    if (c->tokens_on_device != 0 && c->tokens_on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (c->nll_first < 0 || c->nll_first >= h->T || c->nll_count < 0 || (int64_t)c->nll_first + c->nll_count > h->T)
        return fail(h, FSMG_ERR_INVALID, "nll_first must be in [0, max_len) and nll_first + nll_count <= max_len");
    if (c->pass_rows < 0 || c->pass_rows > 1024) return fail(h, FSMG_ERR_INVALID, "pass_rows must be 0 or in [1, 1024]");
    if (!tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    if (!outs[0] && !outs[1] && !outs[2] && !outs[3] && !outs[4]) return fail(h, FSMG_ERR_INVALID, "every output is null");
    return FSMG_OK;
}

// fsmg_score's work at the parameters the handle holds now (no BEGIN_CALL: the MAML variant calls it at theta')
// (`len`: fsmg_score_masked -- the passes are the same launches; the host clears what lies behind a song's end)
int score_core(fsmg_model* h, const fsmg_score_config* c, const int32_t* tokens, float* out_logprob, int32_t* out_rank,
               float* out_entropy, int32_t* out_argmax, float* out_row_nll, const int32_t* len = nullptr) {
    const int R = c->n_rows, T = h->T;
    const int P = c->pass_rows > 0 ? c->pass_rows : FSMG_SCORE_PASS_ROWS;      // a function of the config alone, never of Bcap
    int rc;
    if (!c->tokens_on_device && (rc = check_host_tokens(h, tokens, (size_t)R * T)) != FSMG_OK) return rc;
    if ((rc = ensure_scratch(h, std::min(R, P))) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    // the row NLL is a sum over the log-probs: they come to the host whether the caller asked for them or not
    std::vector<float> lp_own;
    float* lp_host = out_logprob;
    if (out_row_nll && !lp_host) { lp_own.resize((size_t)R * T); lp_host = lp_own.data(); }
    const int mask = (lp_host ? 1 : 0) | (out_rank ? 2 : 0) | (out_entropy ? 4 : 0) | (out_argmax ? 8 : 0);
    // device output k of a pass of B rows (B * T words each): 0 log-prob, 1 entropy (float), 2 rank, 3 argmax (int)
    auto d_out = [&](int B, int k) { return h->score_out + (size_t)k * B * T; };
    rc = run_passes(
        h, tokens, R, P, c->tokens_on_device,
        [&](int, int B) {
            return run_graphed(h, "sc:" + std::to_string(B) + ":" + std::to_string(mask), [&]() -> int {
                int r = token_prep(h, 0, B);
                if (r == FSMG_OK) r = forward(h, B, B, 1, nullptr, false, HEAD_LOGITS);
                if (r != FSMG_OK) return r;
                ScopedTimer tm(h, "ce");
                HIPCK(h, launch_score_rows(h->stream, h->logits, h->V1p, B * T, h->V1, h->Y, B, T, (mask & 1) ? d_out(B, 0) : nullptr,
                                           (mask & 2) ? (int*)d_out(B, 2) : nullptr, (mask & 4) ? d_out(B, 1) : nullptr,
                                           (mask & 8) ? (int*)d_out(B, 3) : nullptr));
                return FSMG_OK;
            });
        },
        [&](int r0, int B) -> int {         // one contiguous block per requested output
            const size_t o = (size_t)r0 * T, bytes = sizeof(float) * (size_t)B * T;
            if (mask & 1) HIPCK(h, hipMemcpyAsync(lp_host + o, d_out(B, 0), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 2) HIPCK(h, hipMemcpyAsync(out_rank + o, d_out(B, 2), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 4) HIPCK(h, hipMemcpyAsync(out_entropy + o, d_out(B, 1), bytes, hipMemcpyDeviceToHost, h->stream));
            if (mask & 8) HIPCK(h, hipMemcpyAsync(out_argmax + o, d_out(B, 3), bytes, hipMemcpyDeviceToHost, h->stream));
            return FSMG_OK;
        });
    if (rc != FSMG_OK) return rc;
    if (len)
        for (int r = 0; r < R; ++r)
            for (size_t i = (size_t)r * T + len[r]; i < (size_t)(r + 1) * T; ++i) {
                if (mask & 1) lp_host[i] = 0.0f;
                if (mask & 2) out_rank[i] = 0;
                if (mask & 4) out_entropy[i] = 0.0f;
                if (mask & 8) out_argmax[i] = 0;
            }
    if (out_row_nll && len) row_nll_masked(lp_host, R, T, c->nll_first, c->nll_count, len, out_row_nll);
    else if (out_row_nll) row_nll(lp_host, R, T, c->nll_first, c->nll_count, out_row_nll);
    return FSMG_OK;
}

}  // namespace

int check_host_lengths(fsmg_model* h, const int32_t* len, size_t n) {
    if (!len) return fail(h, FSMG_ERR_INVALID, "null lengths");
    for (size_t i = 0; i < n; ++i)
        if (len[i] < 1 || len[i] > h->T) return fail(h, FSMG_ERR_INVALID, "every length must be in [1, max_len]");
    return FSMG_OK;
}

void row_nll_masked(const float* logprob, int R, int T, int nll_first, int nll_count, const int32_t* len, float* out) {
    const int t0 = nll_first, t1 = nll_count > 0 ? t0 + nll_count : T;
    for (int r = 0; r < R; ++r) {
        const int te = std::min(t1, (int)len[r]);
        double s = 0.0;
        for (int t = t0; t < te; ++t) s += (double)logprob[(size_t)r * T + t];
        out[r] = te > t0 ? (float)(-s / (double)(te - t0)) : NAN;
    }
}

int check_host_tokens(fsmg_model* h, const int32_t* tokens, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "token id outside [0, input_size)");
    return FSMG_OK;
}

void row_nll(const float* logprob, int R, int T, int nll_first, int nll_count, float* out) {
    const int t0 = nll_first, t1 = nll_count > 0 ? t0 + nll_count : T;
    for (int r = 0; r < R; ++r) {
        double s = 0.0;
        for (int t = t0; t < t1; ++t) s += (double)logprob[(size_t)r * T + t];
        out[r] = (float)(-s / (double)(t1 - t0));
    }
}

int run_passes(fsmg_model* h, const int32_t* tokens, int R, int P, int on_device, const std::function<int(int, int)>& launch,
               const std::function<int(int, int)>& read_back) {
    bool retried = false;
    for (int r0 = 0; r0 < R; r0 += P) {
        const int B = std::min(P, R - r0);
        int rc;
        choose_schedule(h, B);
        h->ov_call = false;             // the projection is one launch behind the last chain whatever order the handle trains with
        if (pass_reads_cs(h, B, false) && (rc = ensure_cs(h)) != FSMG_OK) return rc;
        const int32_t* rows = tokens + (size_t)r0 * h->T;
        if ((rc = stage_tokens(h, rows, 0, rows, B, on_device)) != FSMG_OK) return rc;
        if ((rc = launch(r0, B)) != FSMG_OK) return rc;
        h->lastB = B;
        if ((rc = read_back(r0, B)) != FSMG_OK) return rc;
        int err = 0;                    // the outputs, then what went wrong: one synchronisation per pass
        HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (!err) { retried = false; continue; }
        HIPCK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));
        if (err == 2) on_timeout(h);
        rc = report(h, err);
        if (!is_retry(rc) || !h->retry_armed || retried) return rc;
        // a persistent kernel could not get its blocks resident: the handle has switched to one launch per time step; repeat this
        // pass that way, as fsmg_eval_batch does
        h->retry_armed = false;
        retried = true;
        r0 -= P;
    }
    return FSMG_OK;
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_score(fsmg_handle h, const fsmg_score_config* c, const int32_t* tokens, float* out_logprob, int32_t* out_rank,
               float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    const void* outs[5] = {out_logprob, out_rank, out_entropy, out_argmax, out_row_nll};
    const int rc = check_score_config(h, c, tokens, outs);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, c, tokens, out_logprob, out_rank, out_entropy, out_argmax, out_row_nll);
}

int fsmg_score_masked(fsmg_handle h, const fsmg_score_config* c, const int32_t* tokens, const int32_t* lengths, float* out_logprob,
                      int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    const void* outs[5] = {out_logprob, out_rank, out_entropy, out_argmax, out_row_nll};
    int rc = check_score_config(h, c, tokens, outs);
    if (rc == FSMG_OK) rc = check_host_lengths(h, lengths, (size_t)c->n_rows);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, c, tokens, out_logprob, out_rank, out_entropy, out_argmax, out_row_nll, lengths);
}

int fsmg_maml_score(fsmg_handle h, const fsmg_score_config* c, const int32_t* support, int32_t n_support_rows, int32_t inner_steps,
                    float inner_lr, int32_t support_on_device, const int32_t* tokens, float* out_logprob, int32_t* out_rank,
                    float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    const void* outs[5] = {out_logprob, out_rank, out_entropy, out_argmax, out_row_nll};
    const int rc = check_score_config(h, c, tokens, outs);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return score_core(h, c, tokens, out_logprob, out_rank, out_entropy, out_argmax, out_row_nll); });
}

// the adaptation over the positions inside a support song only; `lengths` (host, NULL: none) are the scored songs' own
// and treat the outputs as fsmg_score_masked does
int fsmg_maml_score_masked(fsmg_handle h, const fsmg_score_config* c, const int32_t* support, const int32_t* support_len, int32_t n_support_rows,
                           int32_t inner_steps, float inner_lr, int32_t support_on_device, const int32_t* tokens, const int32_t* lengths,
                           float* out_logprob, int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    const void* outs[5] = {out_logprob, out_rank, out_entropy, out_argmax, out_row_nll};
    int rc = check_score_config(h, c, tokens, outs);
    if (rc == FSMG_OK && lengths) rc = check_host_lengths(h, lengths, (size_t)c->n_rows);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return score_core(h, c, tokens, out_logprob, out_rank, out_entropy, out_argmax, out_row_nll, lengths); },
                              support_len, true);
}

}  // extern "C"
