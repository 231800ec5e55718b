// Scoring of given songs: fsmg_score and fsmg_maml_score (at theta', through with_adapted_theta in api_step.hip).
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernel lives in score.hip.  DESIGN.md 15.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

namespace {

int check_score_config(fsmg_model* h, const fsmg_score_config* c, const int32_t* tokens, const void* const outs[5]) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_score_config");
    if (c->version != FSMG_SCORE_CONFIG_VERSION)
        return fail(h, FSMG_ERR_INVALID, "fsmg_score_config.version is " + std::to_string(c->version) + ", this library expects " +
                                             std::to_string(FSMG_SCORE_CONFIG_VERSION));
    for (int32_t r : c->reserved)
        if (r != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_score_config.reserved must be zero");
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
int score_core(fsmg_model* h, const fsmg_score_config* c, const int32_t* tokens, float* out_logprob, int32_t* out_rank,
               float* out_entropy, int32_t* out_argmax, float* out_row_nll) {
    const int R = c->n_rows, T = h->T;
    const int P = c->pass_rows > 0 ? c->pass_rows : FSMG_SCORE_PASS_ROWS;      // a function of the config alone, never of Bcap
    if (!c->tokens_on_device) {         // a host song is range-checked before any device work
        for (size_t i = 0, n = (size_t)R * T; i < n; ++i)
            if (tokens[i] < 0 || tokens[i] >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "token id outside [0, input_size)");
    }
    int rc = ensure_scratch(h, std::min(R, P));
    if (rc != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    // the row NLL is a sum over the log-probs: they come to the host whether the caller asked for them or not
    std::vector<float> lp_own;
    float* lp_host = out_logprob;
    if (out_row_nll && !lp_host) { lp_own.resize((size_t)R * T); lp_host = lp_own.data(); }
    const int mask = (lp_host ? 1 : 0) | (out_rank ? 2 : 0) | (out_entropy ? 4 : 0) | (out_argmax ? 8 : 0);
    bool retried = false;
    for (int r0 = 0; r0 < R; r0 += P) {
        const int B = std::min(P, R - r0);
        const size_t n = (size_t)B * T;
        choose_schedule(h, B);
        h->ov_call = false;             // the projection is one launch behind the last chain whatever order the handle trains with
        if (pass_reads_cs(h, B, false) && (rc = ensure_cs(h)) != FSMG_OK) return rc;
        const int32_t* q = tokens + (size_t)r0 * T;
        if ((rc = stage_tokens(h, q, 0, q, B, c->tokens_on_device)) != FSMG_OK) return rc;
        float* d_lp = h->score_out;
        float* d_ent = d_lp + n;
        int* d_rank = (int*)(d_ent + n);
        int* d_arg = d_rank + n;
        rc = run_graphed(h, "sc:" + std::to_string(B) + ":" + std::to_string(mask), [&]() -> int {
            int r = token_prep(h, 0, B);
            if (r == FSMG_OK) r = forward(h, B, B, 1, nullptr, false, HEAD_LOGITS);
            if (r != FSMG_OK) return r;
            ScopedTimer tm(h, "ce");
            HIPCK(h, launch_score_rows(h->stream, h->logits, h->V1p, (int)n, h->V1, h->Y, B, T, (mask & 1) ? d_lp : nullptr,
                                       (mask & 2) ? d_rank : nullptr, (mask & 4) ? d_ent : nullptr, (mask & 8) ? d_arg : nullptr));
            return FSMG_OK;
        });
        if (rc != FSMG_OK) return rc;
        h->lastB = B;
        // one contiguous block per requested output, then what went wrong: one synchronisation per pass
        const size_t o = (size_t)r0 * T;
        int err = 0;
        if (mask & 1) HIPCK(h, hipMemcpyAsync(lp_host + o, d_lp, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        if (mask & 2) HIPCK(h, hipMemcpyAsync(out_rank + o, d_rank, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        if (mask & 4) HIPCK(h, hipMemcpyAsync(out_entropy + o, d_ent, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
        if (mask & 8) HIPCK(h, hipMemcpyAsync(out_argmax + o, d_arg, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        if (err) {
            HIPCK(h, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));
            if (err == 2) on_timeout(h);
            rc = report(h, err);
            if (is_retry(rc) && h->retry_armed && !retried) {
                // a persistent kernel could not get its blocks resident: the handle has switched to one launch per time step;
                // repeat this pass that way, as fsmg_eval_batch does
                h->retry_armed = false;
                retried = true;
                r0 -= P;
                continue;
            }
            return rc;
        }
        retried = false;
    }
    if (out_row_nll) {
        const int t0 = c->nll_first, t1 = c->nll_count > 0 ? t0 + c->nll_count : T;
        for (int r = 0; r < R; ++r) {
            double s = 0.0;             // fp64, increasing t, rounded once: bitwise recomputable from out_logprob
            for (int t = t0; t < t1; ++t) s += (double)lp_host[(size_t)r * T + t];
            out_row_nll[r] = (float)(-s / (double)(t1 - t0));
        }
    }
    return FSMG_OK;
}

}  // namespace

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

}  // extern "C"
