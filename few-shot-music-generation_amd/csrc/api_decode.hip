// Batched on-device decoding: fsmg_generate / fsmg_generate_filtered, fsmg_beam_search, their MAML twins (at theta', through
// with_adapted_theta in api_step.hip) and fsmg_sample, the one-row greedy case of the generate driver; and the decode states
// (fsmg_dstate_*): the same driver started from a carried LSTM state and committed back to it.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in decode.hip.  DESIGN.md 12-14, 16.
#include <memory>

#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

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

namespace {
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
    int* flag = nullptr;                                      // one word behind the output block: fsmg_dstate_feed's token-range flag
    size_t extra_bytes = 0;                                   // set by the caller: a block of its own behind everything else
    char* extra = nullptr;                                    // (cache-conditioned generation: the cache kernels' scratch)
};

// One constrained call's constraint side: the object, the caller's state arrays, the host block
// [state R | dead_ends R | open R * KW] the rows' states are loaded from and read back into, and the device tables with the rows'
// working state, which begin_decode places in the call's scratch.
struct ConRun {
    const fsmg_constraint_s* c = nullptr;
    fsmg_constraint_state* io = nullptr;
    int R = 0;
    std::vector<int32_t> host;
    ConstraintDev dev{};
    ConstraintDev alt{};            // beam search: the second buffer of the rows' states (a new slot gathers its parent's)
    int* row_dead = nullptr;        // beam search: [R], this position's dead-end rows
    size_t bytes() const { return sizeof(int32_t) * host.size(); }
};

// The prologue of generate (W = 0) and beam search (W > 0: W rows per primer row): a host primer is range-checked before any device
// work; the scratch is laid out (h->gen grown if need be); the token buffer rows get [start word, primer row]; a device primer is
// checked once, before the token loop; the LSTM state is zeroed.
// From a decode state (st != nullptr; P = st->kept()) the three differences of a stateful call: the primer region of the token rows
// is the state's history tail, so that the pending token sits at position P, where the caller's loop starts; h and c are copied
// from the state (row r from state row r / W); and `primer` is nullptr, or with `feed` the call's [R][num] given tokens (ids in
// [0, input_size]), which go behind the tail -- a device array's range flag is d.flag, read back with the outputs.
int begin_decode(fsmg_model* h, Decode& d, int R, int W, int P, int num, bool primer_on_device, const int32_t* primer,
                 const fsmg_dstate_s* st = nullptr, bool feed = false, ConRun* cr = nullptr) {
    const bool beam = W > 0;
    const int rows_per_primer = beam ? W : 1;
    const size_t n_primer = st ? (feed ? (size_t)R * num : 0) : (size_t)(R / rows_per_primer) * P;
    if (n_primer > 0 && !primer_on_device) {
        const int hi = st ? h->V1 : h->V;           // fed tokens may be the start word
        for (size_t i = 0; i < n_primer; ++i)
            if (primer[i] < 0 || primer[i] >= hi)
                return fail(h, FSMG_ERR_TOKEN_RANGE, st ? "fed id outside [0, input_size]" : "primer id outside [0, input_size)");
    }
    d.R = R; d.P = P; d.num = num;
    d.ldl = (int)round_up(h->V1, 64);
    d.ldtok = P + num + 1;
    const size_t layer = (size_t)h->L * R * h->Hp, n = (size_t)R * num, cands = (size_t)R * W;
    Carver cv;
    const size_t o_state = cv.take(sizeof(float) * layer * (beam ? 4 : 3));
    const size_t o_logits = cv.take(sizeof(float) * R * d.ldl);
    const size_t o_tok = cv.take(sizeof(int) * R * d.ldtok);
    const size_t o_beam = cv.take(beam ? sizeof(float) * (R + 3 * cands + 3 * n) : 0);
    const size_t o_out = cv.take(sizeof(float) * (2 * n + (beam ? R : 0) + 1));
    const size_t o_primer = cv.take(sizeof(int) * n_primer);
    const size_t o_err = cv.take(sizeof(int));
    const size_t o_extra = cv.take(d.extra_bytes);
    const size_t o_con = cv.take(cr ? cr->bytes() : 0);
    const size_t o_con_alt = cv.take(cr && beam ? cr->bytes() + sizeof(int) * R : 0);
    int rc = gen_reserve(h, cv.off);
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
    d.flag = (int*)(d.out_score + (beam ? R : 0));
    int* err = (int*)(base + o_err);
    d.extra = base + o_extra;

    hipStream_t s = h->stream;
    const int32_t* d_primer = primer;
    if (n_primer > 0 && !primer_on_device) {
        d_primer = (const int32_t*)(base + o_primer);
        HIPCK(h, hipMemcpyAsync((void*)d_primer, primer, sizeof(int) * n_primer, hipMemcpyHostToDevice, s));
    }
    if (cr) {       // the rows' constraint states: loaded here, walked over the primer below
        cr->dev.state = (int*)(base + o_con);
        cr->dev.dead = cr->dev.state + R;
        cr->dev.open = (unsigned*)(cr->dev.dead + R);
        HIPCK(h, hipMemcpyAsync(cr->dev.state, cr->host.data(), cr->bytes(), hipMemcpyHostToDevice, s));
        if (beam) {
            cr->alt = cr->dev;
            cr->alt.state = (int*)(base + o_con_alt);
            cr->alt.dead = cr->alt.state + R;
            cr->alt.open = (unsigned*)(cr->alt.dead + R);
            cr->row_dead = (int*)(cr->alt.open + (size_t)R * cr->dev.KW);
        }
    }
    if (st) {
        HIPCK(h, launch_dstate_rows(s, h->L, R, st->R, h->Hp, nullptr, rows_per_primer, st->h, d.h_in, st->c, d.c, st->ctx, st->history + 1, 0,
                                    d.tok, d.ldtok, 0, P + 1));
        if (feed) {
            HIPCK(h, hipMemsetAsync(d.flag, 0, sizeof(int), s));
            HIPCK(h, launch_dstate_tokens(s, d_primer, R, num, h->V1, h->V, d.tok, d.ldtok, P + 1, d.flag));
        }
        return FSMG_OK;
    }
    HIPCK(h, hipMemsetAsync(err, 0, sizeof(int), s));
    HIPCK(h, launch_gen_primer(s, d_primer, R, P, h->V, h->V, d.tok, d.ldtok, err, rows_per_primer));
    if (cr && P > 0) HIPCK(h, launch_constraint_advance(s, cr->dev, h->V1, R, P, d.tok, d.ldtok, err));
    if (P > 0 && primer_on_device) {
        int e = 0;
        HIPCK(h, hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        if (e) return fail(h, FSMG_ERR_TOKEN_RANGE, cr ? "primer id outside [0, input_size), or not allowed by the constraint where it stands"
                                                       : "primer id outside [0, input_size)");
    }
    HIPCK(h, hipMemsetAsync(d.h_in, 0, sizeof(float) * layer, s));
    HIPCK(h, hipMemsetAsync(d.c, 0, sizeof(float) * layer, s));
    return FSMG_OK;
}

// The end of a stateful call that read `n` tokens behind the state's tail: h (the cells' last output, in d.h_in after the loop's
// swap), c and the new history tail go back to the state; the counters move on the host.
int commit_state(fsmg_model* h, const Decode& d, fsmg_dstate_s* st, int n, bool generated) {
    const int keep = (int)std::min<long long>(st->n_ctx + n, st->history);
    HIPCK(h, launch_dstate_rows(h->stream, h->L, d.R, d.R, h->Hp, nullptr, 1, d.h_in, st->h, d.c, st->c, d.tok, d.ldtok, d.P + n - keep + 1,
                                st->ctx, st->history + 1, 1, keep));
    st->n_ctx += n;
    if (generated) st->n_gen += n;
    return FSMG_OK;
}

// Every layer one position p (it reads tok[:, p]): layer l reads h_in[l] and the new h of the layer below, writes h_out[l] and
// updates c[l].  At a generated position (p >= P), or wherever fsmg_dstate_feed wants a log-prob, the top layer's h_out then gives
// the logits.
int advance(fsmg_model* h, const Decode& d, int p, bool logits) {
    const size_t layer = (size_t)d.R * h->Hp;
    const float* x = nullptr;
    for (int l = 0; l < h->L; ++l) {
        HIPCK(h, launch_gen_cell(h->stream, h->P + h->off_kx[l], h->in_dim[l], h->P + h->off_kh[l], h->P + h->off_b[l], h->Hp,
                                 l == 0 ? h->P + h->off_emb : nullptr, h->Ep, d.tok, d.ldtok, p, x, d.h_in + l * layer, d.h_out + l * layer,
                                 d.c + l * layer, d.R));
        x = d.h_out + l * layer;
    }
    if (logits) HIPCK(h, launch_gen_logits(h->stream, h->P + h->off_w, h->V1p, h->P + h->off_d, h->V1, x, h->Hp, d.R, d.logits, d.ldl));
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
    const int rc = check_config_header(h, c, name, version);
    if (rc != FSMG_OK) return rc;
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
    const int rc = check_config_header(h, f, "fsmg_gen_filters", FSMG_GEN_FILTERS_VERSION);
    if (rc != FSMG_OK) return rc;
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

// ---- constrained decoding
// the constraint `con` if this handle owns it (the registry: a destroyed or foreign pointer is never dereferenced)
fsmg_constraint_s* find_constraint(fsmg_model* h, fsmg_constraint con) {
    for (fsmg_constraint_s* c : h->constraints)
        if (c == con && con != nullptr) return c;
    fail(h, FSMG_ERR_INVALID, "not a constraint of this handle (never created here, or already destroyed)");
    return nullptr;
}

// is token v allowed in (s, open)?  the host twin of decode.hip's con_allowed; *nx = the next state
bool con_allowed_host(const fsmg_constraint_s& c, int s, const uint32_t* open, int v, int* nx) {
    *nx = c.h_next[(size_t)s * c.C + c.h_cls[(size_t)v]];
    if (!(c.h_bias[(size_t)v] > -INFINITY) || *nx < 0) return false;
    const unsigned w = c.h_slot[(size_t)v];
    if (w == 0u) return true;
    const unsigned k = (w & 0x7FFFFFFFu) - 1u;
    return ((open[k >> 5] >> (k & 31u)) & 1u) == (w >> 31);
}

// What a constrained call checks before any device work: the caller's state arrays (NULL: start state, every slot closed, zero dead
// ends) -> cr.host, and a host primer walked from there -- an id outside [0, input_size) is the twin's FSMG_ERR_TOKEN_RANGE, a token
// that is not allowed where it stands FSMG_ERR_INVALID.  The device walks the primer again from the same block.
int con_prepare(fsmg_model* h, ConRun& cr, const fsmg_constraint_s* c, fsmg_constraint_state* io, int R, const int32_t* host_primer, int P) {
    cr.c = c; cr.io = io; cr.R = R;
    const size_t KW = (size_t)c->KW;
    cr.host.assign((size_t)R * (2 + KW), 0);
    int32_t* state = cr.host.data();
    int32_t* dead = state + R;
    uint32_t* open = (uint32_t*)(dead + R);
    for (int b = 0; b < R; ++b) {
        state[b] = io && io->state ? io->state[b] : c->start;
        dead[b] = io && io->dead_ends ? io->dead_ends[b] : 0;
        if (state[b] < 0 || state[b] >= c->S) return fail(h, FSMG_ERR_INVALID, "cstate_io.state outside [0, n_states)");
        if (dead[b] < 0) return fail(h, FSMG_ERR_INVALID, "cstate_io.dead_ends must be >= 0");
        for (size_t i = 0; io && io->open && i < KW; ++i) {
            const uint32_t w = io->open[(size_t)b * KW + i];
            const int live = c->K - 32 * (int)i;      // the slots of this word
            if (live < 32 && (w >> live) != 0u) return fail(h, FSMG_ERR_INVALID, "cstate_io.open has a bit at or above n_slots");
            open[(size_t)b * KW + i] = w;
        }
    }
    cr.dev = ConstraintDev{c->bias, c->cls, c->slot, c->next, c->S, c->C, c->KW, nullptr, nullptr, nullptr};
    if (!host_primer || P <= 0) return FSMG_OK;
    std::vector<uint32_t> o(KW + 1);
    for (int b = 0; b < R; ++b) {
        int s = state[b];
        std::copy(open + (size_t)b * KW, open + (size_t)(b + 1) * KW, o.begin());
        for (int p = 0; p < P; ++p) {
            const int v = host_primer[(size_t)b * P + p];
            if (v < 0 || v >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
            int nx = 0;
            if (!con_allowed_host(*c, s, o.data(), v, &nx))
                return fail(h, FSMG_ERR_INVALID, "primer token " + std::to_string(p) + " of row " + std::to_string(b) +
                                                     " is not allowed by the constraint where it stands");
            s = nx;
            const unsigned w = c->h_slot[(size_t)v];
            if (w != 0u) { const unsigned k = (w & 0x7FFFFFFFu) - 1u; o[k >> 5] ^= 1u << (k & 31u); }
        }
    }
    return FSMG_OK;
}

// the rows' states back into cr.host (one copy, behind the token loop on the stream); done: wait for it and hand it to the caller
void con_scatter(ConRun& cr) {
    if (!cr.io) return;
    const size_t R = (size_t)cr.R;
    const int32_t* state = cr.host.data();
    if (cr.io->state) std::memcpy(cr.io->state, state, sizeof(int32_t) * R);
    if (cr.io->dead_ends) std::memcpy(cr.io->dead_ends, state + R, sizeof(int32_t) * R);
    if (cr.io->open && cr.c->KW > 0) std::memcpy(cr.io->open, state + 2 * R, sizeof(uint32_t) * R * cr.c->KW);
}
int con_read_back(fsmg_model* h, ConRun& cr, bool done) {
    HIPCK(h, hipMemcpyAsync(cr.host.data(), cr.dev.state, cr.bytes(), hipMemcpyDeviceToHost, h->stream));
    if (!done) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));
    con_scatter(cr);
    return FSMG_OK;
}

// fsmg_generate_filtered's work at the parameters the handle holds now (no BEGIN_CALL: the MAML variants call it at theta').
// f == nullptr or neutral: fsmg_generate's pick.  st != nullptr: from that decode state (the token loop starts at the pending token,
// the Philox position runs on from n_gen) and back into it.  cg != nullptr (fsmg_cache_generate with lambda > 0): at every generated
// position the logits rows are overwritten with the mixed log-probabilities z'' before the unchanged pick reads them.
int generate_core(fsmg_model* h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer, int32_t* out_tokens,
                  float* out_logprob, fsmg_dstate_s* st = nullptr, CacheGen* cg = nullptr, ConRun* cr = nullptr) {
    const bool neutral = !f || ((f->top_p == 0.f || f->top_p == 1.f) && f->min_p == 0.f &&
                                (f->repetition_penalty == 0.f || f->repetition_penalty == 1.f));
    GenFilters pf{};
    if (!neutral) pf = GenFilters{f->top_p, f->min_p, f->repetition_penalty == 0.f ? 1.f : f->repetition_penalty, f->repeat_window};
    const GenFilters* pick_f = neutral ? nullptr : &pf;      // neutral filters: exactly fsmg_generate's pick
    Decode d;
    if (cg && g->num > 0) d.extra_bytes = cache_gen_bytes(h, *cg);        // the scratch grows here, never inside the token loop
    int rc = begin_decode(h, d, g->n_seq, 0, st ? st->kept() : g->primer_len, g->num, g->primer_on_device, primer, st, false, cr);
    if (rc != FSMG_OK) return rc;
    if (d.num == 0) return cr ? con_read_back(h, *cr, true) : rc;
    if (cg && (rc = cache_gen_place(h, *cg, d.extra)) != FSMG_OK) return rc;
    const int p0 = st ? d.P : 0, ctr0 = st ? (int)st->n_gen : 0;
    // position p reads tok[:, p]; primer positions (p < P) run the cells only, generated position t = p - P writes tok[:, p + 1]
    for (int p = p0; p < d.P + d.num; ++p) {
        if ((rc = advance(h, d, p, p >= d.P)) != FSMG_OK) return rc;
        // the rows' queries: the top layer's h_out of this position, whose projection the logits are
        const float* top = d.h_out + (size_t)(h->L - 1) * d.R * h->Hp;
        if (cg && cg->W > 0) {      // the self-cache: every position files its key, primer positions included; entry e's value is tok[e + 1]
            if ((rc = cache_self_file(h, *cg, top, p)) != FSMG_OK) return rc;
            if (p >= d.P && (rc = cache_self_step(h, *cg, p, top, d.logits, d.tok + 1, d.ldtok, nullptr)) != FSMG_OK) return rc;
        } else if (p >= d.P && cg && (rc = cache_gen_step(h, *cg, d.h_out + (size_t)(h->L - 1) * d.R * h->Hp, d.logits, nullptr)) != FSMG_OK) return rc;
        if (p >= d.P && cr)
            HIPCK(h, launch_gen_pick_constrained(h->stream, d.logits, d.ldl, h->V1, d.R, g->temperature, g->top_k, pick_f, cr->dev, g->seed,
                                                 p - d.P, ctr0 + p - d.P, d.tok, d.ldtok, p + 1, d.out_tok, d.out_lp, d.num));
        else if (p >= d.P)
            HIPCK(h, launch_gen_pick(h->stream, d.logits, d.ldl, h->V1, d.R, g->temperature, g->top_k, pick_f, g->seed, p - d.P,
                                     ctr0 + p - d.P, d.tok, d.ldtok, p + 1, d.out_tok, d.out_lp, d.num));
        std::swap(d.h_in, d.h_out);                 // the new state is every row's own
    }
    if (st && (rc = commit_state(h, d, st, d.num, true)) != FSMG_OK) return rc;
    if (cr && (rc = con_read_back(h, *cr, false)) != FSMG_OK) return rc;
    if ((rc = read_outputs(h, d, out_tokens, out_logprob)) != FSMG_OK) return rc;
    if (cr) con_scatter(*cr);
    return FSMG_OK;
}

// fsmg_beam_search's work at the parameters the handle holds now (no BEGIN_CALL, as generate_core).  st != nullptr: group g starts
// from row g of that decode state, which is only read.
int beam_core(fsmg_model* h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob,
              const fsmg_dstate_s* st = nullptr, ConRun* cr = nullptr) {
    const int G = b->n_groups, W = b->beam_width, L = h->L, Hp = h->Hp;
    hipStream_t s = h->stream;
    Decode d;
    // the primer runs on all G * W rows (row r reads primer[r / W]): the slots of a group stay identical until the first pick
    int rc = begin_decode(h, d, G * W, W, st ? st->kept() : b->primer_len, b->num, b->primer_on_device, primer, st, false, cr);
    if (rc != FSMG_OK) return rc;
    HIPCK(h, launch_beam_init(s, d.cum, d.R, W));
    // position p reads tok[:, p]; generated position t = p - P writes tok[:, p + 1] and par / htok / hlp [t]
    for (int p = st ? d.P : 0; p < d.P + d.num; ++p) {
        if ((rc = advance(h, d, p, p >= d.P)) != FSMG_OK) return rc;
        if (p < d.P) {                              // no choice yet: the new state is every row's own
            std::swap(d.h_in, d.h_out);
            continue;
        }
        const size_t t = p - d.P, at = t * d.R;
        if (cr) {       // the ranking over the allowed sets; every new slot takes its parent's constraint state, at the last position too
            HIPCK(h, launch_beam_rowtop_constrained(s, d.logits, d.ldl, h->V1, d.R, W, d.cum, cr->dev, d.cand_s, d.cand_lp, d.cand_v,
                                                    cr->row_dead));
            HIPCK(h, launch_beam_select_constrained(s, G, W, h->V1, d.cand_s, d.cand_lp, d.cand_v, cr->row_dead, cr->dev, cr->alt.state,
                                                    cr->alt.dead, d.cum, d.tok, d.ldtok, p + 1, d.par + at, d.htok + at, d.hlp + at));
            HIPCK(h, launch_beam_con_reorder(s, d.R, W, cr->dev, d.par + at, d.htok + at, cr->row_dead, cr->alt.open));
            std::swap(cr->dev, cr->alt);
        } else {
            HIPCK(h, launch_beam_rowtop(s, d.logits, d.ldl, h->V1, d.R, W, d.cum, d.cand_s, d.cand_lp, d.cand_v));
            HIPCK(h, launch_beam_select(s, G, W, h->V1, d.cand_s, d.cand_lp, d.cand_v, d.cum, d.tok, d.ldtok, p + 1, d.par + at, d.htok + at,
                                        d.hlp + at));
        }
        if ((int)t + 1 < d.num) {                   // each slot continues from its parent's state
            HIPCK(h, launch_beam_reorder(s, L, d.R, W, Hp, d.par + at, d.h_out, d.h_in, d.c, d.c_spare));
            std::swap(d.c, d.c_spare);
        }
    }
    HIPCK(h, launch_beam_backtrace(s, d.R, W, d.num, d.par, d.htok, d.hlp, d.cum, d.out_tok, d.out_lp, d.out_score));
    if (cr && (rc = con_read_back(h, *cr, false)) != FSMG_OK) return rc;
    if ((rc = read_outputs(h, d, out_tokens, out_logprob, out_scores)) != FSMG_OK) return rc;
    if (cr) con_scatter(*cr);
    return FSMG_OK;
}

// What a constrained beam call checks before any device work: con_prepare over the G groups' states and host primers, then every
// group's state replicated over its W rows; the final states of the G * W hypotheses go to cstate_out.
int beam_con_prepare(fsmg_model* h, ConRun& cr, const fsmg_constraint_s* c, const fsmg_constraint_state* in, fsmg_constraint_state* out,
                     const fsmg_beam_config* b, const int32_t* host_primer) {
    fsmg_constraint_state io{};
    if (in) io = *in;               // (only read: con_scatter runs on `out`)
    const int G = b->n_groups, W = b->beam_width, R = G * W;
    const int rc = con_prepare(h, cr, c, in ? &io : nullptr, G, host_primer, b->primer_len);
    if (rc != FSMG_OK) return rc;
    const size_t KW = (size_t)c->KW;
    const std::vector<int32_t> grp = cr.host;
    cr.host.assign((size_t)R * (2 + KW), 0);
    for (int r = 0; r < R; ++r) {
        const int g = r / W;
        cr.host[r] = grp[g];
        cr.host[(size_t)R + r] = grp[(size_t)G + g];
        for (size_t i = 0; i < KW; ++i) cr.host[2 * (size_t)R + r * KW + i] = grp[2 * (size_t)G + g * KW + i];
    }
    cr.R = R;
    cr.io = out;
    return FSMG_OK;
}

// fsmg_dstate_feed's work: the n given tokens behind the state's tail; position p reads tok[:, p] (the pending token first) and, with
// log-probs, scores tok[:, p + 1] from its output.  One D2H copy: the log-probs and the device tokens' range flag.
int feed_core(fsmg_model* h, fsmg_dstate_s* st, const int32_t* tokens, int n, bool on_device, float* out_logprob) {
    Decode d;
    int rc = begin_decode(h, d, st->R, 0, st->kept(), n, on_device, tokens, st, true);
    if (rc != FSMG_OK) return rc;
    for (int p = d.P; p < d.P + n; ++p) {
        if ((rc = advance(h, d, p, out_logprob != nullptr)) != FSMG_OK) return rc;
        if (out_logprob)
            HIPCK(h, launch_feed_logprob(h->stream, d.logits, d.ldl, h->V1, d.R, d.tok, d.ldtok, p + 1, d.out_lp, n, p - d.P));
        std::swap(d.h_in, d.h_out);
    }
    if ((rc = commit_state(h, d, st, n, false)) != FSMG_OK) return rc;
    if (!out_logprob && !on_device) {               // host tokens were checked up front: nothing to read back, but the caller's
        HIPCK(h, hipStreamSynchronize(h->stream));  // array must have been consumed before the call returns
        return FSMG_OK;
    }
    const size_t nlp = out_logprob ? (size_t)d.R * n : 0;
    std::vector<float> host(nlp + 1);
    if (out_logprob) {              // [out_lp | flag] are contiguous (generate's layout with no beam scores)
        HIPCK(h, hipMemcpyAsync(host.data(), d.out_lp, sizeof(float) * (nlp + 1), hipMemcpyDeviceToHost, h->stream));
    } else {
        HIPCK(h, hipMemcpyAsync(host.data(), d.flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    int bad = 0;
    std::memcpy(&bad, host.data() + nlp, sizeof(int));
    if (on_device && bad) return fail(h, FSMG_ERR_TOKEN_RANGE, "fed id outside [0, input_size] (the state's contents are unspecified now)");
    if (out_logprob) std::memcpy(out_logprob, host.data(), sizeof(float) * nlp);
    return FSMG_OK;
}

// the decode state `st` if this handle owns it (the registry: a destroyed or foreign pointer is never dereferenced)
fsmg_dstate_s* find_state(fsmg_model* h, fsmg_dstate st) {
    for (fsmg_dstate_s* s : h->dstates)
        if (s == st && st != nullptr) return s;
    fail(h, FSMG_ERR_INVALID, "not a decode state of this handle (never created here, or already destroyed)");
    return nullptr;
}

int reset_state(fsmg_model* h, fsmg_dstate_s* st) {
    HIPCK(h, launch_dstate_reset(h->stream, (long long)h->L * st->R * h->Hp, st->h, st->c, (long long)st->R * (st->history + 1), st->ctx, h->V));
    st->n_ctx = st->n_gen = 0;
    return FSMG_OK;
}

// rows * (history + n + 1) token slots of a stateful call over n tokens: the one-shot calls' bound
bool state_call_fits(const fsmg_dstate_s* st, int64_t rows, int64_t n) { return rows * ((int64_t)st->history + n + 1) <= (1LL << 30); }

// what fsmg_dstate_generate refuses, before any device work
int check_state_generate(fsmg_model* h, const fsmg_dstate_s* s, const fsmg_gen_config* g, const fsmg_gen_filters* f, int32_t* out_tokens) {
    int rc = check_gen_config(h, g, nullptr, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    if (g->n_seq != s->R) return fail(h, FSMG_ERR_INVALID, "n_seq must be the state's row count");
    if (g->primer_len != 0) return fail(h, FSMG_ERR_INVALID, "primer_len must be 0 with a decode state (feed the primer)");
    if (!state_call_fits(s, s->R, g->num)) return fail(h, FSMG_ERR_INVALID, "rows * (history + num + 1) too large");
    if (s->n_gen + g->num > INT32_MAX) return fail(h, FSMG_ERR_INVALID, "n_gen + num exceeds 2^31 - 1");
    if (f && f->repetition_penalty != 0.f && f->repetition_penalty != 1.f) {      // the penalty must find its whole window in the history
        if (f->repeat_window > s->history) return fail(h, FSMG_ERR_INVALID, "repeat_window must be in [1, history]");
        if (f->repeat_window == 0 && s->n_ctx + g->num > s->history)
            return fail(h, FSMG_ERR_INVALID, "repeat_window 0 (the whole context) needs n_ctx + num <= history");
    }
    return FSMG_OK;
}

// fsmg_cache_generate / fsmg_dstate_cache_generate behind the argument checks.  lambda = 0: the plain driver, the cache not read
// (and its value index not built).  The tiles' host arrays in cg must outlive the uploads: a failed call is synchronised too.
int cache_generate_core(fsmg_model* h, CacheGen& cg, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer,
                        int32_t* out_tokens, float* out_logprob, fsmg_dstate_s* st) {
    if (cg.lambda == 0.0f) return generate_core(h, g, f, primer, out_tokens, out_logprob, st);
    int rc = cg.c ? ensure_value_index(h, const_cast<fsmg_cache_s*>(cg.c)) : FSMG_OK;
    if (rc != FSMG_OK) return rc;
    rc = generate_core(h, g, f, primer, out_tokens, out_logprob, st, &cg);
    if (rc != FSMG_OK) hipStreamSynchronize(h->stream);
    return rc;
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

// the adaptation over the positions inside a support song only; the generation at theta' is fsmg_maml_generate_filtered's
int fsmg_maml_generate_filtered_masked(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* support,
                                       const int32_t* support_len, int32_t n_support_rows, int32_t inner_steps, float inner_lr,
                                       int32_t support_on_device, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return generate_core(h, g, f, primer, out_tokens, out_logprob); }, support_len, true);
}

// ---- constrained decoding
int fsmg_constraint_create(fsmg_handle h, const fsmg_constraint_config* c, fsmg_constraint* out) {
    if (!h) return FSMG_ERR_INVALID;
    if (!c || !out) return fail(h, FSMG_ERR_INVALID, "null fsmg_constraint_config / out");
    int rc = check_config_header(h, c, "fsmg_constraint_config", FSMG_CONSTRAINT_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (c->n_columns != h->V1) return fail(h, FSMG_ERR_INVALID, "n_columns must be input_size + 1 of this handle");
    if (h->V1 > (1 << 19)) return fail(h, FSMG_ERR_INVALID, "a constraint needs input_size + 1 <= 2^19");   // (two bitmaps of an unstaged row in LDS)
    const bool automaton = c->token_class || c->next_state;
    if (automaton && !(c->token_class && c->next_state)) return fail(h, FSMG_ERR_INVALID, "token_class and next_state come together");
    if (!automaton && (c->n_states != 0 || c->n_classes != 0 || c->start_state != 0))
        return fail(h, FSMG_ERR_INVALID, "without an automaton n_states, n_classes and start_state must be 0");
    const int S = automaton ? c->n_states : 1, Cn = automaton ? c->n_classes : 1, K = c->n_slots, V1 = h->V1;
    if (S < 1 || S > CON_MAX_STATES) return fail(h, FSMG_ERR_INVALID, "n_states must be in [1, 256]");
    if (Cn < 1 || Cn > CON_MAX_CLASSES) return fail(h, FSMG_ERR_INVALID, "n_classes must be in [1, 64]");
    if (K < 0 || K > CON_MAX_SLOTS) return fail(h, FSMG_ERR_INVALID, "n_slots must be in [0, 4096]");
    if (c->start_state < 0 || c->start_state >= S) return fail(h, FSMG_ERR_INVALID, "start_state outside [0, n_states)");
    fsmg_constraint_s* con = new (std::nothrow) fsmg_constraint_s;
    if (!con) return fail(h, FSMG_ERR_NOMEM, "out of host memory");
    std::unique_ptr<fsmg_constraint_s> guard(con);
    con->V1 = V1; con->S = S; con->C = Cn; con->K = K; con->KW = (K + 31) / 32; con->start = c->start_state;
    con->h_bias.assign((size_t)V1, 0.0f);
    con->h_cls.assign((size_t)V1, 0);
    con->h_slot.assign((size_t)V1, 0u);
    con->h_next.assign((size_t)S * Cn, 0);
    for (int v = 0; v < V1; ++v) {
        if (c->bias) {
            const float bv = c->bias[v];
            if (bv != bv || bv == INFINITY) return fail(h, FSMG_ERR_INVALID, "bias must be finite or -inf");
            con->h_bias[(size_t)v] = bv;
        }
        if (automaton) {
            if (c->token_class[v] < 0 || c->token_class[v] >= Cn) return fail(h, FSMG_ERR_INVALID, "token_class outside [0, n_classes)");
            con->h_cls[(size_t)v] = (unsigned char)c->token_class[v];
        }
        const int so = c->slot_open ? c->slot_open[v] : -1, sc = c->slot_close ? c->slot_close[v] : -1;
        if (so < -1 || so >= K || sc < -1 || sc >= K) return fail(h, FSMG_ERR_INVALID, "slot index outside [-1, n_slots)");
        if (so >= 0 && sc >= 0) return fail(h, FSMG_ERR_INVALID, "a token both opens and closes a slot");
        if (so >= 0) con->h_slot[(size_t)v] = (unsigned)(so + 1);
        if (sc >= 0) con->h_slot[(size_t)v] = (unsigned)(sc + 1) | 0x80000000u;
    }
    for (size_t i = 0; automaton && i < (size_t)S * Cn; ++i) {
        if (c->next_state[i] < -1 || c->next_state[i] >= S) return fail(h, FSMG_ERR_INVALID, "next_state outside [-1, n_states)");
        con->h_next[i] = (short)c->next_state[i];
    }
    BEGIN_CALL(h);
    Carver cv;
    const size_t o_bias = cv.take(sizeof(float) * V1), o_slot = cv.take(sizeof(unsigned) * V1), o_next = cv.take(sizeof(short) * S * Cn),
                 o_cls = cv.take((size_t)V1);
    if (hipMalloc((void**)&con->mem, cv.off) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(constraint) failed");
    con->bias = (float*)(con->mem + o_bias);
    con->slot = (unsigned*)(con->mem + o_slot);
    con->next = (short*)(con->mem + o_next);
    con->cls = (unsigned char*)(con->mem + o_cls);
    hipError_t e = hipMemcpyAsync(con->bias, con->h_bias.data(), sizeof(float) * V1, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(con->slot, con->h_slot.data(), sizeof(unsigned) * V1, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(con->next, con->h_next.data(), sizeof(short) * S * Cn, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(con->cls, con->h_cls.data(), (size_t)V1, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        hipFree(con->mem);
        return fail(h, FSMG_ERR_HIP, std::string("uploading the constraint: ") + hipGetErrorString(e));
    }
    h->constraints.push_back(guard.release());
    *out = con;
    return FSMG_OK;
}

int fsmg_constraint_destroy(fsmg_handle h, fsmg_constraint con) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    HIPCK(h, hipStreamSynchronize(h->stream));      // nothing in flight reads it
    h->constraints.erase(std::find(h->constraints.begin(), h->constraints.end(), c));
    hipFree(c->mem);
    delete c;
    return FSMG_OK;
}

int fsmg_constraint_info(fsmg_handle h, fsmg_constraint con, int64_t out[4]) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    if (!out) return fail(h, FSMG_ERR_INVALID, "null out");
    out[0] = c->V1; out[1] = c->S; out[2] = c->C; out[3] = c->K;
    return FSMG_OK;
}

int fsmg_generate_constrained(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, fsmg_constraint con,
                              fsmg_constraint_state* cstate_io, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!con) return fsmg_generate_filtered(h, g, f, primer, out_tokens, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    ConRun cr;
    if (rc == FSMG_OK) rc = con_prepare(h, cr, c, cstate_io, g->n_seq, g->primer_on_device ? nullptr : primer, g->primer_len);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, f, primer, out_tokens, out_logprob, nullptr, nullptr, &cr);
}

int fsmg_maml_generate_constrained(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, fsmg_constraint con,
                                   fsmg_constraint_state* cstate_io, const int32_t* support, const int32_t* support_len,
                                   int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                   const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!con)
        return support_len ? fsmg_maml_generate_filtered_masked(h, g, f, support, support_len, n_support_rows, inner_steps, inner_lr,
                                                                support_on_device, primer, out_tokens, out_logprob)
                           : fsmg_maml_generate_filtered(h, g, f, support, n_support_rows, inner_steps, inner_lr, support_on_device, primer,
                                                         out_tokens, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    ConRun cr;
    if (rc == FSMG_OK) rc = con_prepare(h, cr, c, cstate_io, g->n_seq, g->primer_on_device ? nullptr : primer, g->primer_len);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return generate_core(h, g, f, primer, out_tokens, out_logprob, nullptr, nullptr, &cr); }, support_len,
                              support_len != nullptr);
}

// the adaptation by dynamic evaluation over the support stream; the generation at theta_l is fsmg_generate_filtered's
int fsmg_dyneval_generate(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* support, const int32_t* support_len,
                          int32_t n_support_rows, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer,
                          int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    return with_dyneval_theta(h, cfg, support, support_len, n_support_rows, [&] { return generate_core(h, g, f, primer, out_tokens, out_logprob); });
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

int fsmg_maml_beam_search_masked(fsmg_handle h, const fsmg_beam_config* b, const int32_t* support, const int32_t* support_len,
                                 int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                 const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    const int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return beam_core(h, b, primer, out_tokens, out_scores, out_logprob); }, support_len, true);
}

// ---- constrained beam search; con == NULL: the unconstrained twin itself
int fsmg_beam_search_constrained(fsmg_handle h, const fsmg_beam_config* b, fsmg_constraint con, const fsmg_constraint_state* cstate_in,
                                 fsmg_constraint_state* cstate_out, const int32_t* primer, int32_t* out_tokens, float* out_scores,
                                 float* out_logprob) {
    if (!con) return fsmg_beam_search(h, b, primer, out_tokens, out_scores, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    ConRun cr;
    if (rc == FSMG_OK) rc = beam_con_prepare(h, cr, c, cstate_in, cstate_out, b, b->primer_on_device ? nullptr : primer);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return beam_core(h, b, primer, out_tokens, out_scores, out_logprob, nullptr, &cr);
}

int fsmg_maml_beam_search_constrained(fsmg_handle h, const fsmg_beam_config* b, fsmg_constraint con, const fsmg_constraint_state* cstate_in,
                                      fsmg_constraint_state* cstate_out, const int32_t* support, const int32_t* support_len,
                                      int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                      const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob) {
    if (!con)
        return support_len ? fsmg_maml_beam_search_masked(h, b, support, support_len, n_support_rows, inner_steps, inner_lr, support_on_device,
                                                          primer, out_tokens, out_scores, out_logprob)
                           : fsmg_maml_beam_search(h, b, support, n_support_rows, inner_steps, inner_lr, support_on_device, primer, out_tokens,
                                                   out_scores, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    ConRun cr;
    if (rc == FSMG_OK) rc = beam_con_prepare(h, cr, c, cstate_in, cstate_out, b, b->primer_on_device ? nullptr : primer);
    if (rc != FSMG_OK) return rc;
    return with_adapted_theta(h, support, n_support_rows, inner_steps, inner_lr, support_on_device,
                              [&] { return beam_core(h, b, primer, out_tokens, out_scores, out_logprob, nullptr, &cr); }, support_len,
                              support_len != nullptr);
}

// ---- decode states
int fsmg_dstate_create(fsmg_handle h, const fsmg_dstate_config* c, fsmg_dstate* out) {
    if (!h) return FSMG_ERR_INVALID;
    if (!c || !out) return fail(h, FSMG_ERR_INVALID, "null fsmg_dstate_config / out");
    int rc = check_config_header(h, c, "fsmg_dstate_config", FSMG_DSTATE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (c->n_rows < 1 || c->n_rows > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n_rows must be in [1, 2^20]");
    if (c->history < 1 || (int64_t)c->n_rows * ((int64_t)c->history + 1) > (1LL << 30))
        return fail(h, FSMG_ERR_INVALID, "history must be >= 1 and n_rows * (history + 1) <= 2^30");
    BEGIN_CALL(h);
    fsmg_dstate_s* st = new (std::nothrow) fsmg_dstate_s;
    if (!st) return fail(h, FSMG_ERR_NOMEM, "out of host memory");
    st->R = c->n_rows; st->history = c->history;
    const size_t layer = (size_t)round_up((int64_t)sizeof(float) * h->L * st->R * h->Hp, 256);
    const size_t bytes = 2 * layer + sizeof(int) * (size_t)st->R * (st->history + 1);
    if (hipMalloc((void**)&st->mem, bytes) != hipSuccess) { delete st; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(decode state) failed"); }
    st->h = (float*)st->mem;
    st->c = (float*)(st->mem + layer);
    st->ctx = (int*)(st->mem + 2 * layer);
    rc = reset_state(h, st);
    if (rc != FSMG_OK) { hipFree(st->mem); delete st; return rc; }
    h->dstates.push_back(st);
    *out = st;
    return FSMG_OK;
}

int fsmg_dstate_destroy(fsmg_handle h, fsmg_dstate st) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    HIPCK(h, hipStreamSynchronize(h->stream));      // nothing in flight reads it
    h->dstates.erase(std::find(h->dstates.begin(), h->dstates.end(), s));
    hipFree(s->mem);
    delete s;
    return FSMG_OK;
}

int fsmg_dstate_reset(fsmg_handle h, fsmg_dstate st) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    return reset_state(h, s);
}

int fsmg_dstate_info(fsmg_handle h, fsmg_dstate st, int64_t out[4]) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    if (!out) return fail(h, FSMG_ERR_INVALID, "null out");
    out[0] = s->R; out[1] = s->history; out[2] = s->n_ctx; out[3] = s->n_gen;
    return FSMG_OK;
}

int fsmg_dstate_get(fsmg_handle h, fsmg_dstate st, float* h_out, float* c_out, int32_t* ctx_out) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    const size_t rows = (size_t)h->L * s->R, ld = (size_t)s->history + 1;
    const int keep = s->kept();
    std::vector<float> hp(rows * h->Hp), cp(rows * h->Hp);
    std::vector<int> ctx((size_t)s->R * ld);
    HIPCK(h, hipMemcpyAsync(hp.data(), s->h, sizeof(float) * hp.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(cp.data(), s->c, sizeof(float) * cp.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync(ctx.data(), s->ctx, sizeof(int) * ctx.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    for (size_t r = 0; r < rows; ++r) {             // the padded units stay inside
        if (h_out) std::memcpy(h_out + r * h->H, hp.data() + r * h->Hp, sizeof(float) * h->H);
        if (c_out) std::memcpy(c_out + r * h->H, cp.data() + r * h->Hp, sizeof(float) * h->H);
    }
    if (ctx_out)
        for (int r = 0; r < s->R; ++r) std::memcpy(ctx_out + (size_t)r * keep, ctx.data() + r * ld + 1, sizeof(int) * keep);
    return FSMG_OK;
}

int fsmg_dstate_set(fsmg_handle h, fsmg_dstate st, const float* h_in, const float* c_in, const int32_t* ctx_in, int64_t n_ctx,
                    int64_t n_gen) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    if (!h_in || !c_in) return fail(h, FSMG_ERR_INVALID, "null h_in / c_in");
    if (n_ctx < 0 || n_gen < 0 || n_gen > n_ctx || n_gen > INT32_MAX) return fail(h, FSMG_ERR_INVALID, "0 <= n_gen <= n_ctx, n_gen < 2^31");
    const int keep = (int)std::min<int64_t>(n_ctx, s->history);
    if (keep > 0 && !ctx_in) return fail(h, FSMG_ERR_INVALID, "n_ctx > 0 needs ctx_in");
    for (size_t i = 0; i < (size_t)s->R * keep; ++i)
        if (ctx_in[i] < 0 || ctx_in[i] >= h->V1) return fail(h, FSMG_ERR_TOKEN_RANGE, "ctx_in id outside [0, input_size]");
    BEGIN_CALL(h);
    const size_t rows = (size_t)h->L * s->R, ld = (size_t)s->history + 1;
    std::vector<float> hp(rows * h->Hp, 0.0f), cp(rows * h->Hp, 0.0f);
    std::vector<int> ctx((size_t)s->R * ld, h->V);
    for (size_t r = 0; r < rows; ++r) {
        std::memcpy(hp.data() + r * h->Hp, h_in + r * h->H, sizeof(float) * h->H);
        std::memcpy(cp.data() + r * h->Hp, c_in + r * h->H, sizeof(float) * h->H);
    }
    for (int r = 0; r < s->R; ++r)
        if (keep > 0) std::memcpy(ctx.data() + r * ld + 1, ctx_in + (size_t)r * keep, sizeof(int) * keep);
    HIPCK(h, hipMemcpyAsync(s->h, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(s->c, cp.data(), sizeof(float) * cp.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(s->ctx, ctx.data(), sizeof(int) * ctx.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));      // the host vectors go out of scope
    s->n_ctx = n_ctx; s->n_gen = n_gen;
    return FSMG_OK;
}

int fsmg_dstate_gather(fsmg_handle h, fsmg_dstate dst, fsmg_dstate src, const int32_t* rows) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* d = find_state(h, dst);
    fsmg_dstate_s* s = d ? find_state(h, src) : nullptr;
    if (!d || !s) return FSMG_ERR_INVALID;
    if (d == s) return fail(h, FSMG_ERR_INVALID, "gather needs dst != src");
    if (d->history != s->history) return fail(h, FSMG_ERR_INVALID, "gather needs states of equal history");
    if (!rows) return fail(h, FSMG_ERR_INVALID, "null rows");
    for (int i = 0; i < d->R; ++i)
        if (rows[i] < 0 || rows[i] >= s->R) return fail(h, FSMG_ERR_INVALID, "gather index outside [0, src rows)");
    BEGIN_CALL(h);
    int rc = gen_reserve(h, sizeof(int) * (size_t)d->R);
    if (rc != FSMG_OK) return rc;
    int* d_rows = (int*)h->gen;
    HIPCK(h, hipMemcpyAsync(d_rows, rows, sizeof(int) * (size_t)d->R, hipMemcpyHostToDevice, h->stream));
    HIPCK(h, launch_dstate_rows(h->stream, h->L, d->R, s->R, h->Hp, d_rows, 1, s->h, d->h, s->c, d->c, s->ctx, s->history + 1, 0, d->ctx,
                                d->history + 1, 0, d->history + 1));
    HIPCK(h, hipStreamSynchronize(h->stream));      // the caller's index array has been consumed
    d->n_ctx = s->n_ctx; d->n_gen = s->n_gen;
    return FSMG_OK;
}

int fsmg_dstate_feed(fsmg_handle h, fsmg_dstate st, const int32_t* tokens, int32_t n, int32_t tokens_on_device, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    if (n < 0) return fail(h, FSMG_ERR_INVALID, "n must be >= 0");
    if (tokens_on_device != 0 && tokens_on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (n > 0 && !tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    if (!state_call_fits(s, s->R, n)) return fail(h, FSMG_ERR_INVALID, "rows * (history + n + 1) too large");
    if (n == 0) return FSMG_OK;
    BEGIN_CALL(h);
    return feed_core(h, s, tokens, n, tokens_on_device != 0, out_logprob);
}

int fsmg_dstate_generate(fsmg_handle h, fsmg_dstate st, const fsmg_gen_config* g, const fsmg_gen_filters* f, int32_t* out_tokens,
                         float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    const int rc = check_state_generate(h, s, g, f, out_tokens);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, f, nullptr, out_tokens, out_logprob, s);
}

// fsmg_dstate_generate under a constraint: the caller's cstate_io is the rows' constraint state from call to call
int fsmg_dstate_generate_constrained(fsmg_handle h, fsmg_dstate st, const fsmg_gen_config* g, const fsmg_gen_filters* f, fsmg_constraint con,
                                     fsmg_constraint_state* cstate_io, int32_t* out_tokens, float* out_logprob) {
    if (!con) return fsmg_dstate_generate(h, st, g, f, out_tokens, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_state_generate(h, s, g, f, out_tokens);
    ConRun cr;
    if (rc == FSMG_OK) rc = con_prepare(h, cr, c, cstate_io, g->n_seq, nullptr, 0);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, f, nullptr, out_tokens, out_logprob, s, nullptr, &cr);
}

// ---- cache-conditioned generation: the generate calls with a support-set cache beside the model
int fsmg_cache_generate(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_gen_config* g,
                        const fsmg_gen_filters* f, const int32_t* group, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    if (!find_cache(h, cache)) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    CacheGen cg;
    if (rc == FSMG_OK) rc = cache_gen_check(h, cache, cc, group, g->n_seq, &cg);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return cache_generate_core(h, cg, g, f, primer, out_tokens, out_logprob, nullptr);
}

// the same with the row's own history in the set; cache may be null
int fsmg_cache_self_generate(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                             const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* group, const int32_t* primer,
                             int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    if (cache && !find_cache(h, cache)) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    CacheGen cg;
    if (rc == FSMG_OK) rc = cache_self_gen_check(h, cache, cc, sc, cache ? group : nullptr, g->n_seq, (int64_t)g->primer_len + g->num, false, &cg);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return cache_generate_core(h, cg, g, f, primer, out_tokens, out_logprob, nullptr);
}

int fsmg_dstate_cache_generate(fsmg_handle h, fsmg_dstate st, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_gen_config* g,
                               const fsmg_gen_filters* f, const int32_t* group, int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    if (!find_cache(h, cache)) return FSMG_ERR_INVALID;
    int rc = check_state_generate(h, s, g, f, out_tokens);
    CacheGen cg;
    if (rc == FSMG_OK) rc = cache_gen_check(h, cache, cc, group, g->n_seq, &cg);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return cache_generate_core(h, cg, g, f, nullptr, out_tokens, out_logprob, s);
}

int fsmg_dstate_beam_search(fsmg_handle h, fsmg_dstate st, const fsmg_beam_config* b, int32_t* out_tokens, float* out_scores,
                            float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    const int rc = check_beam_config(h, b, nullptr, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    if (b->n_groups != s->R) return fail(h, FSMG_ERR_INVALID, "n_groups must be the state's row count");
    if (b->primer_len != 0) return fail(h, FSMG_ERR_INVALID, "primer_len must be 0 with a decode state (feed the primer)");
    if (!state_call_fits(s, (int64_t)s->R * b->beam_width, b->num)) return fail(h, FSMG_ERR_INVALID, "rows * beam_width * (history + num + 1) too large");
    BEGIN_CALL(h);
    return beam_core(h, b, nullptr, out_tokens, out_scores, out_logprob, s);
}

// fsmg_dstate_beam_search under a constraint: cstate_in is the groups' constraint state behind what the state has read
int fsmg_dstate_beam_search_constrained(fsmg_handle h, fsmg_dstate st, const fsmg_beam_config* b, fsmg_constraint con,
                                        const fsmg_constraint_state* cstate_in, fsmg_constraint_state* cstate_out, int32_t* out_tokens,
                                        float* out_scores, float* out_logprob) {
    if (!con) return fsmg_dstate_beam_search(h, st, b, out_tokens, out_scores, out_logprob);
    if (!h) return FSMG_ERR_INVALID;
    fsmg_dstate_s* s = find_state(h, st);
    if (!s) return FSMG_ERR_INVALID;
    fsmg_constraint_s* c = find_constraint(h, con);
    if (!c) return FSMG_ERR_INVALID;
    int rc = check_beam_config(h, b, nullptr, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    if (b->n_groups != s->R) return fail(h, FSMG_ERR_INVALID, "n_groups must be the state's row count");
    if (b->primer_len != 0) return fail(h, FSMG_ERR_INVALID, "primer_len must be 0 with a decode state (feed the primer)");
    if (!state_call_fits(s, (int64_t)s->R * b->beam_width, b->num)) return fail(h, FSMG_ERR_INVALID, "rows * beam_width * (history + num + 1) too large");
    ConRun cr;
    rc = beam_con_prepare(h, cr, c, cstate_in, cstate_out, b, nullptr);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return beam_core(h, b, nullptr, out_tokens, out_scores, out_logprob, s, &cr);
}

}  // extern "C"
