// Dynamic evaluation (include/fsmg.h "dynamic evaluation"): the gradient statistics, the streaming driver that scores a
// window before it adapts on it, the entry points.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); every kernel lives in dyneval.hip / elementwise.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

static int64_t logical_elements(const fsmg_model* h) {
    int64_t n = 0;
    for (const auto& p : h->params) n += p.rows * p.cols;
    return n;
}

// the statistics' allocation, zeroed, on first use
static int ensure_dyn_stats(fsmg_model* h) {
    if (h->dyn_stats) return FSMG_OK;
    Carver c;
    const size_t o_ms = c.take(sizeof(float) * (size_t)h->n_flat), o_part = c.take(sizeof(double) * (size_t)dyneval_rms_blocks(h->n_flat)),
                 o_mean = c.take(sizeof(float) * 4);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (hipMalloc((void**)&h->dyn_stats, c.off) != hipSuccess) { h->dyn_stats = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(dynamic-evaluation statistics) failed"); }
    HIPCK(h, hipMemset(h->dyn_stats, 0, c.off));
    h->dyn_ms = (float*)(h->dyn_stats + o_ms); h->dyn_part = (double*)(h->dyn_stats + o_part); h->d_mean_rms = (float*)(h->dyn_stats + o_mean);
    h->dyn_count = 0; h->dyn_rms_dirty = true;
    return FSMG_OK;
}

// d_mean_rms is current: recomputed (stream order, no synchronisation) when the statistics have changed since
static int refresh_mean_rms(fsmg_model* h) {
    if (!h->dyn_rms_dirty) return FSMG_OK;
    if (h->dyn_count <= 0) HIPCK(h, launch_fill32(h->stream, h->d_mean_rms, 0u, 4));
    else HIPCK(h, launch_dyneval_mean_rms(h->stream, h->dyn_ms, h->n_flat, h->dyn_count, logical_elements(h), h->dyn_part, h->d_mean_rms));
    h->dyn_rms_dirty = false;
    return FSMG_OK;
}

static int check_dyneval_config(fsmg_model* h, const fsmg_dyneval_config* c) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_dyneval_config");
    if (c->struct_size != (int32_t)sizeof(fsmg_dyneval_config))
        return fail(h, FSMG_ERR_INVALID, "fsmg_dyneval_config.struct_size is " + std::to_string(c->struct_size) + ", this library expects " +
                                             std::to_string(sizeof(fsmg_dyneval_config)));
    if (c->reserved != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_dyneval_config.reserved must be zero");
    if (c->rule != FSMG_DYNEVAL_SGD && c->rule != FSMG_DYNEVAL_RMS) return fail(h, FSMG_ERR_INVALID, "rule must be FSMG_DYNEVAL_SGD or FSMG_DYNEVAL_RMS");
    if (c->seg_len < 1 || c->seg_len > h->T) return fail(h, FSMG_ERR_INVALID, "seg_len must be in [1, max_len]");
    if (c->rows_per_step < 1 || c->rows_per_step > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "rows_per_step must be in [1, 2^20]");
    if (!(c->lr >= 0.f) || !std::isfinite(c->lr)) return fail(h, FSMG_ERR_INVALID, "lr must be finite and >= 0");
    if (!(c->decay >= 0.f && c->decay <= 1.f)) return fail(h, FSMG_ERR_INVALID, "decay must be in [0, 1]");
    if (c->rule == FSMG_DYNEVAL_RMS && (!(c->eps > 0.f) || !std::isfinite(c->eps))) return fail(h, FSMG_ERR_INVALID, "eps must be finite and > 0 for the RMS rule");
    if (!(c->clip_norm >= 0.f) || !std::isfinite(c->clip_norm)) return fail(h, FSMG_ERR_INVALID, "clip_norm must be finite and >= 0 (0: no clipping)");
    if (c->adapt_reported != 0 && c->adapt_reported != 1) return fail(h, FSMG_ERR_INVALID, "adapt_reported must be 0 or 1");
    return FSMG_OK;
}

// everything a stream is checked for, before any device work; `len` gets the lengths the stream runs with (T where lengths == NULL)
static int check_stream(fsmg_model* h, const fsmg_dyneval_config* c, const int32_t* tokens, const int32_t* lengths, int64_t n_rows,
                        int64_t first_reported, std::vector<int32_t>* len) {
    int rc = check_dyneval_config(h, c);
    if (rc != FSMG_OK) return rc;
    if (!tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    if (n_rows < 1 || n_rows > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n_rows must be in [1, 2^20]");
    if (first_reported < 0 || first_reported > n_rows) return fail(h, FSMG_ERR_INVALID, "first_reported must be in [0, n_rows]");
    if (lengths && (rc = check_host_lengths(h, lengths, (size_t)n_rows)) != FSMG_OK) return rc;
    if ((rc = check_host_tokens(h, tokens, (size_t)n_rows * h->T)) != FSMG_OK) return rc;
    if (c->rule == FSMG_DYNEVAL_RMS && (h->dyn_stats == nullptr || h->dyn_count <= 0))
        return fail(h, FSMG_ERR_STATE, "the RMS rule needs gradient statistics (fsmg_dyneval_stats_accumulate / _set, count > 0)");
    if (len) {
        len->assign((size_t)n_rows, h->T);
        if (lengths) std::copy(lengths, lengths + n_rows, len->begin());
    }
    return FSMG_OK;
}

// the update of one window from the gradient the pass left (sgd_update's shape: norm partials, the fused kernel, the K_h images)
static int dyneval_update(fsmg_model* h, const fsmg_dyneval_config* c) {
    hipStream_t s = h->stream;
    const bool slices = h->cfg.clip_norm_mode == FSMG_CLIP_TF1_SLICES;
    const int64_t skip = slices ? round_up((int64_t)h->V1 * h->Ep, FLAT_ALIGN) : 0;
    const int64_t n = h->n_flat - skip;
    {
        ScopedTimer tm(h, "update");
        HIPCK(h, launch_sqnorm_partials(s, h->G + skip, n, h->partials));
    }
    DynUpdateArgs a{};
    a.p = h->P; a.pg = h->P_saved; a.g = h->G; a.ms = h->dyn_ms; a.n = h->n_flat;
    a.partials = h->partials; a.n_partials = sqnorm_blocks(n); a.tail = h->G + h->n_flat; a.use_slices = slices ? 1 : 0;
    a.rms = c->rule == FSMG_DYNEVAL_RMS ? 1 : 0; a.lr = c->lr; a.decay = c->decay; a.eps = c->eps; a.clip = c->clip_norm;
    a.count = (float)h->dyn_count; a.mean_rms = h->d_mean_rms; a.gnorm_out = h->d_gnorm; a.err_flag = h->d_err;
    {
        ScopedTimer tm(h, "dyneval_update");
        HIPCK(h, launch_dyneval_update(s, a));
    }
    h->khf_dirty = true;
    h->have_grads = false;
    return ensure_khf(h);
}

// the blocks and windows of one stream at theta_l = the handle's parameters (the caller saved theta); d_out: [n_rows][T], zeroed, or nullptr
static int run_stream(fsmg_model* h, const fsmg_dyneval_config* c, const int32_t* tokens, const int32_t* len, int n_rows, int first_reported, float* d_out) {
    const int T = h->T, S = c->seg_len, P = c->rows_per_step;
    int rc = FSMG_OK;
    for (int r0 = 0; r0 < n_rows && rc == FSMG_OK;) {
        // the block ends at the next multiple of rows_per_step, at first_reported, or at the stream's end, whichever comes first
        int r1 = std::min<int64_t>(n_rows, ((int64_t)r0 / P + 1) * P);
        if (r0 < first_reported && first_reported < r1) r1 = first_reported;
        const int nb = r1 - r0;
        const bool reported = r0 >= first_reported;
        const bool adapt = !reported || c->adapt_reported != 0;
        const int seg = adapt ? S : T;
        for (int lo = 0; lo < T && rc == FSMG_OK; lo += seg) {
            const int hi = std::min(lo + seg, T);
            int64_t n_valid = 0;
            for (int b = 0; b < nb; ++b) n_valid += std::max(0, std::min(hi, (int)len[r0 + b]) - lo);
            if (n_valid == 0) continue;
            rc = window_rows_pass(h, tokens + (size_t)r0 * T, len + r0, nb, lo, hi);
            if (rc == FSMG_OK && reported && d_out) HIPCK(h, launch_dyneval_collect(h->stream, h->ce, h->roww, nb, T, r0, d_out));
            if (rc == FSMG_OK && adapt) rc = dyneval_update(h, c);
        }
        r0 = r1;
    }
    h->have_grads = false;
    return rc;
}

static int ensure_dyn_out(fsmg_model* h, int64_t words) {
    if (h->dyn_out_cap >= words) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->dyn_out) { hipFree(h->dyn_out); h->dyn_out = nullptr; h->dyn_out_cap = 0; }
    const int64_t cap = round_up(std::max<int64_t>(words, 4096), 64);
    if (hipMalloc((void**)&h->dyn_out, sizeof(float) * (size_t)cap) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(dynamic-evaluation scores) failed");
    h->dyn_out_cap = cap;
    return FSMG_OK;
}

// One stream from theta: save theta, adapt (scores into host_out [n_rows][T] when it is not null), run `body` at theta_l, put theta
// back whatever happened.  A time-out inside the stream leaves skipped updates behind: theta comes back and the whole stream is
// repeated once on per-step launches.  (arguments checked by the caller; no BEGIN_CALL of its own beyond the passes')
int dyneval_stream(fsmg_model* h, const fsmg_dyneval_config* c, const int32_t* tokens, const int32_t* len, int n_rows, int first_reported,
                   float* host_out, const std::function<int()>* body) {
    const int64_t words = (int64_t)n_rows * h->T;
    return at_adapted_theta(
        h,
        [&]() {             // theta is saved and the mean RMS refreshed inside each attempt: a repeat starts from what the first one started from
            int rc = save_theta(h);
            if (rc == FSMG_OK && c->rule == FSMG_DYNEVAL_RMS) rc = refresh_mean_rms(h);
            if (rc == FSMG_OK && host_out) {
                rc = ensure_dyn_out(h, words);
                if (rc == FSMG_OK) HIPCK(h, launch_fill32(h->stream, h->dyn_out, 0u, round_up(words, 4)));
            }
            if (rc == FSMG_OK) rc = run_stream(h, c, tokens, len, n_rows, first_reported, host_out ? h->dyn_out : nullptr);
            return rc != FSMG_OK ? rc : adapt_flag(h);       // a time-out / token error inside the stream: its updates were skipped
        },
        [&]() {
            const int rc = body ? (*body)() : FSMG_OK;
            if (rc == FSMG_OK && host_out) {
                HIPCK(h, hipMemcpyAsync(host_out, h->dyn_out, sizeof(float) * (size_t)words, hipMemcpyDeviceToHost, h->stream));
                HIPCK(h, hipStreamSynchronize(h->stream));
            }
            return rc;
        });
}

// fsmg_dyneval_generate's adapt-decode-restore (the decode body lives with the decode driver, api_decode.hip)
int with_dyneval_theta(fsmg_model* h, const fsmg_dyneval_config* c, const int32_t* support, const int32_t* support_len, int32_t n_support_rows,
                       const std::function<int()>& at_theta_l) {
    std::vector<int32_t> len;
    const int rc = check_stream(h, c, support, support_len, n_support_rows, n_support_rows, &len);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return dyneval_stream(h, c, support, len.data(), n_support_rows, n_support_rows, nullptr, &at_theta_l);
}

// minus the fp64 sum of logprob[r][0 .. len[r]) for the rows [r0, r1) added to *sum / *count in (row, position) order; row_nll: per row, rounded once
static void sum_rows(const float* logprob, const int32_t* len, int T, int r0, int r1, double* sum, int64_t* count, float* row_nll) {
    for (int r = r0; r < r1; ++r) {
        double s = 0.0;
        for (int t = 0; t < len[r]; ++t) { s += (double)logprob[(size_t)r * T + t]; *sum += (double)logprob[(size_t)r * T + t]; }
        *count += len[r];
        if (row_nll) row_nll[r] = (float)(-s);
    }
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_dyneval_stats_reset(fsmg_handle h) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    h->dyn_count = 0; h->dyn_rms_dirty = true;
    if (!h->dyn_stats) return FSMG_OK;
    HIPCK(h, launch_fill32(h->stream, h->dyn_ms, 0u, h->n_flat));
    return FSMG_OK;
}

int fsmg_dyneval_stats_accumulate(fsmg_handle h) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    if (!h->have_grads) return fail(h, FSMG_ERR_STATE, "fsmg_dyneval_stats_accumulate without a gradient of a preceding fsmg_forward_backward");
    int rc = ensure_dyn_stats(h);
    if (rc != FSMG_OK) return rc;
    // a pass that was skipped on the device (a time-out, a token out of range) left garbage: the flag stays for whoever consumes the gradient
    int err = 0;
    HIPCK(h, hipMemcpyAsync(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (err) return fail(h, FSMG_ERR_STATE, "the pending gradient belongs to a pass that was skipped on the device: nothing accumulated");
    HIPCK(h, launch_dyneval_accumulate(h->stream, h->dyn_ms, h->G, h->n_flat));
    ++h->dyn_count; h->dyn_rms_dirty = true;
    return FSMG_OK;
}

int fsmg_dyneval_stats_info(fsmg_handle h, int64_t* count, float* mean_rms) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    if (count) *count = h->dyn_count;
    if (!mean_rms) return FSMG_OK;
    *mean_rms = 0.0f;
    if (!h->dyn_stats || h->dyn_count <= 0) return FSMG_OK;
    const int rc = refresh_mean_rms(h);
    if (rc != FSMG_OK) return rc;
    HIPCK(h, hipMemcpyAsync(mean_rms, h->d_mean_rms, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return FSMG_OK;
}

int fsmg_dyneval_stats_get(fsmg_handle h, const char* name, float* sum, int64_t n) {
    if (!h || !name || !sum) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    const int rc = ensure_dyn_stats(h);
    if (rc != FSMG_OK) return rc;
    return download_tensor(h, h->dyn_ms, name, sum, n);
}

int fsmg_dyneval_stats_set(fsmg_handle h, const char* name, const float* sum, int64_t n) {
    if (!h || !name || !sum) return FSMG_ERR_INVALID;
    const ParamDesc* p = find_param(h, name);
    if (!p) return fail(h, FSMG_ERR_NAME, std::string("unknown parameter '") + name + "'");
    if (n != p->rows * p->cols) return fail(h, FSMG_ERR_SIZE, std::string("size mismatch for '") + name + "'");
    for (int64_t i = 0; i < n; ++i)
        if (!(sum[i] >= 0.f) || !std::isfinite(sum[i])) return fail(h, FSMG_ERR_INVALID, "a sum of squares must be finite and >= 0");
    BEGIN_CALL(h);
    int rc = ensure_dyn_stats(h);
    if (rc != FSMG_OK) return rc;
    rc = upload_tensor(h, h->dyn_ms, name, sum, n);
    h->dyn_rms_dirty = true;
    return rc;
}

int fsmg_dyneval_stats_set_count(fsmg_handle h, int64_t count) {
    if (!h) return FSMG_ERR_INVALID;
    if (count < 0) return fail(h, FSMG_ERR_INVALID, "count must be >= 0");
    BEGIN_CALL(h);
    const int rc = ensure_dyn_stats(h);
    if (rc != FSMG_OK) return rc;
    h->dyn_count = count; h->dyn_rms_dirty = true;
    return FSMG_OK;
}

int fsmg_dyneval_score(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* tokens, const int32_t* lengths, int32_t n_rows,
                       int32_t first_reported, float* out_logprob, float* out_row_nll, float* out_nll) {
    if (!h) return FSMG_ERR_INVALID;
    std::vector<int32_t> len;
    int rc = check_stream(h, cfg, tokens, lengths, n_rows, first_reported, &len);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    const bool want = out_logprob || out_row_nll || out_nll;
    std::vector<float> own;
    float* lp = out_logprob;
    if (want && !lp) { own.resize((size_t)n_rows * h->T); lp = own.data(); }
    rc = dyneval_stream(h, cfg, tokens, len.data(), n_rows, first_reported, lp, nullptr);
    if (rc != FSMG_OK || !want) return rc;
    double sum = 0.0; int64_t count = 0;
    if (out_row_nll) std::fill(out_row_nll, out_row_nll + first_reported, 0.0f);
    sum_rows(lp, len.data(), h->T, first_reported, n_rows, &sum, &count, out_row_nll);
    if (out_nll) *out_nll = count > 0 ? (float)(-sum / (double)count) : std::nanf("");
    return FSMG_OK;
}

int fsmg_dyneval_eval_step(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* support, const int32_t* query,
                           const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* nll) {
    if (!h) return FSMG_ERR_INVALID;
    if (!support || !query || !nll) return fail(h, FSMG_ERR_INVALID, "null support / query / nll");
    if (K < 1 || Q < 1) return fail(h, FSMG_ERR_INVALID, "K and Q must be >= 1");
    int rc = validate_shape(h, N, K, Q);
    if (rc != FSMG_OK) return rc;
    const int T = h->T, R = K + Q;
    // every artist's stream is checked before the first one runs: a refused call touches nothing
    std::vector<int32_t> tok((size_t)N * R * T), len((size_t)N * R, T);
    for (int n = 0; n < N; ++n) {
        std::copy(support + (size_t)n * K * T, support + (size_t)(n + 1) * K * T, tok.begin() + (size_t)n * R * T);
        std::copy(query + (size_t)n * Q * T, query + (size_t)(n + 1) * Q * T, tok.begin() + ((size_t)n * R + K) * T);
        if (support_len) std::copy(support_len + (size_t)n * K, support_len + (size_t)(n + 1) * K, len.begin() + (size_t)n * R);
        if (query_len) std::copy(query_len + (size_t)n * Q, query_len + (size_t)(n + 1) * Q, len.begin() + (size_t)n * R + K);
    }
    if ((rc = check_stream(h, cfg, tok.data(), len.data(), (int64_t)N * R, 0, nullptr)) != FSMG_OK) return rc;
    BEGIN_CALL(h);
    std::vector<float> lp((size_t)R * T);
    double sum = 0.0; int64_t count = 0;
    for (int n = 0; n < N; ++n) {
        rc = dyneval_stream(h, cfg, tok.data() + (size_t)n * R * T, len.data() + (size_t)n * R, R, K, lp.data(), nullptr);
        if (rc != FSMG_OK) return rc;
        sum_rows(lp.data(), len.data() + (size_t)n * R, T, K, R, &sum, &count, nullptr);
    }
    *nll = (float)(-sum / (double)count);
    return FSMG_OK;
}

}  // extern "C"
