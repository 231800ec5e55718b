// Batched on-device decoding: fsmg_generate / fsmg_generate_filtered, fsmg_beam_search, their MAML twins (at theta', through
// with_adapted_theta in api_step.hip) and fsmg_sample, the one-row greedy case of the generate driver.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in decode.hip.  DESIGN.md 12-14.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

namespace {
// h->gen holds at least `bytes`: grown between calls, after a stream sync
int gen_reserve(fsmg_model* h, size_t bytes) {
    if (bytes <= h->gen_bytes) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));     // never inside the token loop
    if (h->gen) hipFree(h->gen);
    h->gen = nullptr; h->gen_bytes = 0;
    if (hipMalloc((void**)&h->gen, bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(generation scratch) failed");
    h->gen_bytes = bytes;
    return FSMG_OK;
}

// One call's buffers in h->gen for R rows (generate: one per sequence; beam search: W per group).
struct Decode {
    int R = 0, P = 0, num = 0, ldl = 0, ldtok = 0;
    float *h_in = nullptr, *h_out = nullptr, *c = nullptr;   // [L][R][Hp]: the cells read h_in and write h_out, c in place
    float* c_spare = nullptr;                                 // [L][R][Hp]: the beam reorder's target for c
    float* logits = nullptr;                                  // [R][ldl]
    int* tok = nullptr;                                       // [R][P + num + 1]: start word, primer, generated tokens
    float *cum = nullptr, *cand_s = nullptr, *cand_lp = nullptr;   // beam search: [R], [R][W], [R][W]
    int* cand_v = nullptr;                                    // beam search: [R][W]
    int *par = nullptr, *htok = nullptr;                      // beam search: [num][R] per generated position
    float* hlp = nullptr;
    int* out_tok = nullptr;                                   // the packed output block, one D2H copy: tokens [R][num], log-probs
    float *out_lp = nullptr, *out_score = nullptr;            // [R][num], beam scores [R]
};

// The prologue of generate (W = 0) and beam search (W > 0: W rows per primer row): a host primer is range-checked before any device
// work; the scratch is laid out (h->gen grown if need be); the token buffer rows get [start word, primer row]; a device primer is
// checked once, before the token loop; the LSTM state is zeroed.
int begin_decode(fsmg_model* h, Decode& d, int R, int W, int P, int num, bool primer_on_device, const int32_t* primer) {
    const bool beam = W > 0;
    const int rows_per_primer = beam ? W : 1;
    const size_t n_primer = (size_t)(R / rows_per_primer) * P;
    if (P > 0 && !primer_on_device) {
        for (size_t i = 0; i < n_primer; ++i)
            if (primer[i] < 0 || primer[i] >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    d.R = R; d.P = P; d.num = num;
    d.ldl = (int)round_up(h->V1, 64);
    d.ldtok = P + num + 1;
    const size_t layer = (size_t)h->L * R * h->Hp, n = (size_t)R * num, cands = (size_t)R * W;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off = (size_t)round_up((int64_t)(off + bytes), 256); return o; };
    const size_t o_state = place(sizeof(float) * layer * (beam ? 4 : 3));
    const size_t o_logits = place(sizeof(float) * R * d.ldl);
    const size_t o_tok = place(sizeof(int) * R * d.ldtok);
    const size_t o_beam = place(beam ? sizeof(float) * (R + 3 * cands + 3 * n) : 0);
    const size_t o_out = place(sizeof(float) * (2 * n + (beam ? R : 0)));
    const size_t o_primer = place(sizeof(int) * n_primer);
    const size_t o_err = place(sizeof(int));
    int rc = gen_reserve(h, off);
    if (rc != FSMG_OK) return rc;
    char* base = h->gen;
    d.h_in = (float*)(base + o_state);
    d.h_out = d.h_in + layer;
    d.c = d.h_out + layer;
    if (beam) d.c_spare = d.c + layer;
    d.logits = (float*)(base + o_logits);
    d.tok = (int*)(base + o_tok);
    if (beam) {
        d.cum = (float*)(base + o_beam);
        d.cand_s = d.cum + R;
        d.cand_lp = d.cand_s + cands;
        d.cand_v = (int*)(d.cand_lp + cands);
        d.par = d.cand_v + cands;
        d.htok = d.par + n;
        d.hlp = (float*)(d.htok + n);
    }
    d.out_tok = (int*)(base + o_out);
    d.out_lp = (float*)(d.out_tok + n);
    d.out_score = d.out_lp + n;
    int* err = (int*)(base + o_err);

    hipStream_t s = h->stream;
    const int32_t* d_primer = primer;
    if (P > 0 && !primer_on_device) {
        d_primer = (const int32_t*)(base + o_primer);
        HIPCK(h, hipMemcpyAsync((void*)d_primer, primer, sizeof(int) * n_primer, hipMemcpyHostToDevice, s));
    }
    HIPCK(h, hipMemsetAsync(err, 0, sizeof(int), s));
    HIPCK(h, launch_gen_primer(s, d_primer, R, P, h->V, h->V, d.tok, d.ldtok, err, rows_per_primer));
    if (P > 0 && primer_on_device) {
        int e = 0;
        HIPCK(h, hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        if (e) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    HIPCK(h, hipMemsetAsync(d.h_in, 0, sizeof(float) * layer, s));
    HIPCK(h, hipMemsetAsync(d.c, 0, sizeof(float) * layer, s));
    return FSMG_OK;
}

// Every layer one position p (it reads tok[:, p]): layer l reads h_in[l] and the new h of the layer below, writes h_out[l] and
// updates c[l].  At a generated position (p >= P) the top layer's h_out then gives the logits.
int advance(fsmg_model* h, const Decode& d, int p) {
    const size_t layer = (size_t)d.R * h->Hp;
    const float* x = nullptr;
    for (int l = 0; l < h->L; ++l) {
        HIPCK(h, launch_gen_cell(h->stream, h->P + h->off_kx[l], h->in_dim[l], h->P + h->off_kh[l], h->P + h->off_b[l], h->Hp,
                                 l == 0 ? h->P + h->off_emb : nullptr, h->Ep, d.tok, d.ldtok, p, x, d.h_in + l * layer, d.h_out + l * layer,
                                 d.c + l * layer, d.R));
        x = d.h_out + l * layer;
    }
    if (p >= d.P) HIPCK(h, launch_gen_logits(h->stream, h->P + h->off_w, h->V1p, h->P + h->off_d, h->V1, x, h->Hp, d.R, d.logits, d.ldl));
    return FSMG_OK;
}

// The packed output block -> the caller's arrays (out_logprob may be null; out_scores only for beam search): one copy, one sync.
int read_outputs(fsmg_model* h, const Decode& d, int32_t* out_tokens, float* out_logprob, float* out_scores = nullptr) {
    const size_t n = (size_t)d.R * d.num;
    std::vector<char> host(n * (sizeof(int) + sizeof(float)) + (out_scores ? sizeof(float) * d.R : 0));
    HIPCK(h, hipMemcpyAsync(host.data(), d.out_tok, host.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_tokens, host.data(), n * sizeof(int));
    if (out_logprob) std::memcpy(out_logprob, host.data() + n * sizeof(int), n * sizeof(float));
    if (out_scores) std::memcpy(out_scores, host.data() + n * (sizeof(int) + sizeof(float)), sizeof(float) * d.R);
    return FSMG_OK;
}

// The checks fsmg_gen_config and fsmg_beam_config share: version, zero reserved words, primer_on_device, a primer when
// primer_len > 0, and the launches' limits over `rows` decode rows (the grids' y dimension and 32-bit token offsets).
template <class Config>
int check_config_common(fsmg_model* h, const Config* c, const char* name, int32_t version, const int32_t* primer, int64_t rows,
                        const char* rows_name) {
    if (c->version != version)
        return fail(h, FSMG_ERR_INVALID, std::string(name) + ".version is " + std::to_string(c->version) + ", this library expects " +
                                             std::to_string(version));
    for (int32_t r : c->reserved)
        if (r != 0) return fail(h, FSMG_ERR_INVALID, std::string(name) + ".reserved must be zero");
    if (c->primer_on_device != 0 && c->primer_on_device != 1) return fail(h, FSMG_ERR_INVALID, "primer_on_device must be 0 or 1");
    if (c->primer_len > 0 && !primer) return fail(h, FSMG_ERR_INVALID, "primer_len > 0 needs a primer");
    if (rows > (1 << 20) || rows * ((int64_t)c->primer_len + c->num + 1) > (1LL << 30))
        return fail(h, FSMG_ERR_INVALID, std::string(rows_name) + " * (primer_len + num + 1) too large");
    return FSMG_OK;
}

int check_gen_config(fsmg_model* h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens) {
    if (!g) return fail(h, FSMG_ERR_INVALID, "null fsmg_gen_config");
    const int rc = check_config_common(h, g, "fsmg_gen_config", FSMG_GEN_CONFIG_VERSION, primer, g->n_seq, "n_seq");
    if (rc != FSMG_OK) return rc;
    if (g->n_seq < 1 || g->num < 0 || g->primer_len < 0) return fail(h, FSMG_ERR_INVALID, "n_seq must be >= 1, num and primer_len >= 0");
    if (!(g->temperature >= 0.f) || !std::isfinite(g->temperature)) return fail(h, FSMG_ERR_INVALID, "temperature must be finite and >= 0");
    if (g->top_k < 0 || g->top_k > h->V1) return fail(h, FSMG_ERR_INVALID, "top_k must be in [0, input_size + 1]");
    if (g->num > 0 && !out_tokens) return fail(h, FSMG_ERR_INVALID, "null out_tokens");
    return FSMG_OK;
}

int check_gen_filters(fsmg_model* h, const fsmg_gen_filters* f) {
    if (!f) return FSMG_OK;
    if (f->version != FSMG_GEN_FILTERS_VERSION)
        return fail(h, FSMG_ERR_INVALID, "fsmg_gen_filters.version is " + std::to_string(f->version) + ", this library expects " +
                                             std::to_string(FSMG_GEN_FILTERS_VERSION));
    for (int i = 0; i < 8; ++i)
        if (f->reserved[i] != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_gen_filters.reserved must be zero");
    if (!(f->top_p >= 0.f && f->top_p <= 1.f)) return fail(h, FSMG_ERR_INVALID, "top_p must be in [0, 1]");
    if (!(f->min_p >= 0.f && f->min_p <= 1.f)) return fail(h, FSMG_ERR_INVALID, "min_p must be in [0, 1]");
    if (!(f->repetition_penalty >= 0.f) || !std::isfinite(f->repetition_penalty))
        return fail(h, FSMG_ERR_INVALID, "repetition_penalty must be finite and >= 0");
    if (f->repeat_window < 0) return fail(h, FSMG_ERR_INVALID, "repeat_window must be >= 0");
    if (f->repetition_penalty != 0.f && f->repetition_penalty != 1.f && h->V1 > (1 << 20))
        return fail(h, FSMG_ERR_INVALID, "repetition_penalty needs input_size + 1 <= 2^20");
    return FSMG_OK;
}

int check_beam_config(fsmg_model* h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores) {
    if (!b) return fail(h, FSMG_ERR_INVALID, "null fsmg_beam_config");
    const int rc = check_config_common(h, b, "fsmg_beam_config", FSMG_BEAM_CONFIG_VERSION, primer, (int64_t)b->n_groups * b->beam_width,
                                       "n_groups * beam_width");
    if (rc != FSMG_OK) return rc;
    if (b->n_groups < 1 || b->num < 1 || b->primer_len < 0) return fail(h, FSMG_ERR_INVALID, "n_groups and num must be >= 1, primer_len >= 0");
    if (b->beam_width < 1 || b->beam_width > 64) return fail(h, FSMG_ERR_INVALID, "beam_width must be in [1, 64]");
    int64_t seqs = 1;                               // V1^num, stopped once it reaches W (no overflow)
    for (int t = 0; t < b->num && seqs < b->beam_width; ++t) seqs *= h->V1;
    if (seqs < b->beam_width) return fail(h, FSMG_ERR_INVALID, "beam_width exceeds the (input_size + 1)^num distinct sequences");
    if (!out_tokens || !out_scores) return fail(h, FSMG_ERR_INVALID, "null out_tokens / out_scores");
    return FSMG_OK;
}

// fsmg_generate_filtered's work at the parameters the handle holds now (no BEGIN_CALL: the MAML variants call it at theta').
// f == nullptr or neutral: fsmg_generate's pick.
int generate_core(fsmg_model* h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer, int32_t* out_tokens,
                  float* out_logprob) {
    const bool neutral = !f || ((f->top_p == 0.f || f->top_p == 1.f) && f->min_p == 0.f &&
                                (f->repetition_penalty == 0.f || f->repetition_penalty == 1.f));
    GenFilters pf{};
    if (!neutral) pf = GenFilters{f->top_p, f->min_p, f->repetition_penalty == 0.f ? 1.f : f->repetition_penalty, f->repeat_window};
    const GenFilters* pick_f = neutral ? nullptr : &pf;      // neutral filters: exactly fsmg_generate's pick
    Decode d;
    int rc = begin_decode(h, d, g->n_seq, 0, g->primer_len, g->num, g->primer_on_device, primer);
    if (rc != FSMG_OK || d.num == 0) return rc;
    // position p reads tok[:, p]; primer positions (p < P) run the cells only, generated position t = p - P writes tok[:, p + 1]
    for (int p = 0; p < d.P + d.num; ++p) {
        if ((rc = advance(h, d, p)) != FSMG_OK) return rc;
        if (p >= d.P)
            HIPCK(h, launch_gen_pick(h->stream, d.logits, d.ldl, h->V1, d.R, g->temperature, g->top_k, pick_f, g->seed, p - d.P, d.tok,
                                     d.ldtok, p + 1, d.out_tok, d.out_lp, d.num));
        std::swap(d.h_in, d.h_out);                 // the new state is every row's own
    }
    return read_outputs(h, d, out_tokens, out_logprob);
}

// fsmg_beam_search's work at the parameters the handle holds now (no BEGIN_CALL, as generate_core)
int beam_core(fsmg_model* h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob) {
    const int G = b->n_groups, W = b->beam_width, L = h->L, Hp = h->Hp;
    hipStream_t s = h->stream;
    Decode d;
    // the primer runs on all G * W rows (row r reads primer[r / W]): the slots of a group stay identical until the first pick
    int rc = begin_decode(h, d, G * W, W, b->primer_len, b->num, b->primer_on_device, primer);
    if (rc != FSMG_OK) return rc;
    HIPCK(h, launch_beam_init(s, d.cum, d.R, W));
    // position p reads tok[:, p]; generated position t = p - P writes tok[:, p + 1] and par / htok / hlp [t]
    for (int p = 0; p < d.P + d.num; ++p) {
        if ((rc = advance(h, d, p)) != FSMG_OK) return rc;
        if (p < d.P) {                              // no choice yet: the new state is every row's own
            std::swap(d.h_in, d.h_out);
            continue;
        }
        const size_t t = p - d.P, at = t * d.R;
        HIPCK(h, launch_beam_rowtop(s, d.logits, d.ldl, h->V1, d.R, W, d.cum, d.cand_s, d.cand_lp, d.cand_v));
        HIPCK(h, launch_beam_select(s, G, W, h->V1, d.cand_s, d.cand_lp, d.cand_v, d.cum, d.tok, d.ldtok, p + 1, d.par + at, d.htok + at,
                                    d.hlp + at));
        if ((int)t + 1 < d.num) {                   // each slot continues from its parent's state
            HIPCK(h, launch_beam_reorder(s, L, d.R, W, Hp, d.par + at, d.h_out, d.h_in, d.c, d.c_spare));
            std::swap(d.c, d.c_spare);
        }
    }
    HIPCK(h, launch_beam_backtrace(s, d.R, W, d.num, d.par, d.htok, d.hlp, d.cum, d.out_tok, d.out_lp, d.out_score));
    return read_outputs(h, d, out_tokens, out_logprob, out_scores);
}
}  // namespace

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

// greedy (temperature 0, no top_k, no primer) on one row
int fsmg_sample(fsmg_handle h, int32_t num, int32_t* out_tokens) {
    if (!h || num < 0 || (num > 0 && !out_tokens)) return FSMG_ERR_INVALID;
    fsmg_gen_config g{};
    g.version = FSMG_GEN_CONFIG_VERSION;
    g.n_seq = 1;
    g.num = num;
    return fsmg_generate(h, &g, nullptr, out_tokens, nullptr);
}

int fsmg_generate(fsmg_handle h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    return fsmg_generate_filtered(h, g, nullptr, primer, out_tokens, out_logprob);
}

int fsmg_generate_filtered(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer, int32_t* out_tokens,
                           float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, f, primer, out_tokens, out_logprob);
}

int fsmg_maml_generate(fsmg_handle h, const fsmg_gen_config* g, const int32_t* support, int32_t n_support_rows, int32_t inner_steps,
                       float inner_lr, int32_t support_on_device, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    return fsmg_maml_generate_filtered(h, g, nullptr, support, n_support_rows, inner_steps, inner_lr, support_on_device, primer, out_tokens,
                                       out_logprob);
}

int fsmg_maml_generate_filtered(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* support,
                                int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return generate_core(h, g, f, primer, out_tokens, out_logprob); });
}

int fsmg_beam_search(fsmg_handle h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores,
                     float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    const int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return beam_core(h, b, primer, out_tokens, out_scores, out_logprob);
}

int fsmg_maml_beam_search(fsmg_handle h, const fsmg_beam_config* b, const int32_t* support, int32_t n_support_rows, int32_t inner_steps,
                          float inner_lr, int32_t support_on_device, const int32_t* primer, int32_t* out_tokens, float* out_scores,
                          float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    const int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return beam_core(h, b, primer, out_tokens, out_scores, out_logprob); });
}

}  // extern "C"
