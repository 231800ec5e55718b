// Batched on-device generation (fsmg_generate; fsmg_maml_generate lives beside fsmg_maml_eval in api_step.hip).
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in decode.hip.  DESIGN.md "Batched generation".
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

namespace {
constexpr size_t GEN_ALIGN = 256;
size_t gen_align(size_t n) { return (n + GEN_ALIGN - 1) / GEN_ALIGN * GEN_ALIGN; }

// one call's scratch: h ping/pong + c per layer, the logits rows, the token buffer [B][P+num+1], the outputs (tokens then
// log-probs, one contiguous D2H copy), a staged host primer, the primer error flag
struct GenLayout {
    size_t state, logits, tok, out_tok, out_lp, primer, err, total;
    int ldl, ldtok;
};
GenLayout gen_layout(const fsmg_model* h, int B, int P, int num) {
    GenLayout g{};
    g.ldl = (int)round_up(h->V1, 64);
    g.ldtok = P + num + 1;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += gen_align(bytes); return o; };
    g.state = place(sizeof(float) * (size_t)h->L * 3 * B * h->Hp);
    g.logits = place(sizeof(float) * (size_t)B * g.ldl);
    g.tok = place(sizeof(int) * (size_t)B * g.ldtok);
    g.out_tok = off;                                       // out_tok and out_lp back to back: one copy
    off += sizeof(int) * (size_t)B * num;
    g.out_lp = off;
    off = gen_align(off + sizeof(float) * (size_t)B * num);
    g.primer = place(sizeof(int) * (size_t)B * P);
    g.err = place(sizeof(int));
    g.total = off;
    return g;
}
}  // namespace

int gen_reserve(fsmg_model* h, size_t bytes) {
    if (bytes <= h->gen_bytes) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));     // grown between calls, never inside the token loop
    if (h->gen) hipFree(h->gen);
    h->gen = nullptr; h->gen_bytes = 0;
    if (hipMalloc((void**)&h->gen, bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(generation scratch) failed");
    h->gen_bytes = bytes;
    return FSMG_OK;
}

int check_gen_config(fsmg_model* h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens) {
    if (!g) return fail(h, FSMG_ERR_INVALID, "null fsmg_gen_config");
    if (g->version != FSMG_GEN_CONFIG_VERSION)
        return fail(h, FSMG_ERR_INVALID, "fsmg_gen_config.version is " + std::to_string(g->version) + ", this library expects " +
                                             std::to_string(FSMG_GEN_CONFIG_VERSION));
    for (int i = 0; i < 7; ++i)
        if (g->reserved[i] != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_gen_config.reserved must be zero");
    if (g->n_seq < 1 || g->num < 0 || g->primer_len < 0) return fail(h, FSMG_ERR_INVALID, "n_seq must be >= 1, num and primer_len >= 0");
    if (!(g->temperature >= 0.f) || !std::isfinite(g->temperature)) return fail(h, FSMG_ERR_INVALID, "temperature must be finite and >= 0");
    if (g->top_k < 0 || g->top_k > h->V1) return fail(h, FSMG_ERR_INVALID, "top_k must be in [0, input_size + 1]");
    if (g->primer_on_device != 0 && g->primer_on_device != 1) return fail(h, FSMG_ERR_INVALID, "primer_on_device must be 0 or 1");
    if (g->primer_len > 0 && !primer) return fail(h, FSMG_ERR_INVALID, "primer_len > 0 needs a primer");
    if (g->num > 0 && !out_tokens) return fail(h, FSMG_ERR_INVALID, "null out_tokens");
    // (the grids' y dimension and 32-bit token offsets)
    if (g->n_seq > (1 << 20) || (int64_t)g->n_seq * ((int64_t)g->primer_len + g->num + 1) > (1LL << 30))
        return fail(h, FSMG_ERR_INVALID, "n_seq * (primer_len + num + 1) too large");
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

bool gen_filters_neutral(const fsmg_gen_filters* f) {
    return !f || ((f->top_p == 0.f || f->top_p == 1.f) && f->min_p == 0.f && (f->repetition_penalty == 0.f || f->repetition_penalty == 1.f));
}

int generate_core(fsmg_model* h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens, float* out_logprob,
                  const fsmg_gen_filters* f) {
    if (gen_filters_neutral(f)) f = nullptr;       // neutral filters: exactly fsmg_generate's pick
    const int B = g->n_seq, P = g->primer_len, num = g->num, L = h->L, Hp = h->Hp;
    if (P > 0 && !g->primer_on_device) {           // a host primer is checked before any device work
        for (int64_t i = 0; i < (int64_t)B * P; ++i)
            if (primer[i] < 0 || primer[i] >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    hipStream_t s = h->stream;
    const GenLayout lay = gen_layout(h, B, P, num);
    const int rc = gen_reserve(h, lay.total);
    if (rc != FSMG_OK) return rc;
    char* base = h->gen;
    float* hb = (float*)(base + lay.state);                       // [L][2][B][Hp]
    float* cb = hb + (size_t)L * 2 * B * Hp;                      // [L][B][Hp]
    float* logits = (float*)(base + lay.logits);
    int* tok = (int*)(base + lay.tok);
    int* out_tok = (int*)(base + lay.out_tok);
    float* out_lp = (float*)(base + lay.out_lp);
    int* err = (int*)(base + lay.err);

    const int32_t* d_primer = primer;
    if (P > 0 && !g->primer_on_device) {
        d_primer = (const int32_t*)(base + lay.primer);
        HIPCK(h, hipMemcpyAsync((void*)d_primer, primer, sizeof(int) * (size_t)B * P, hipMemcpyHostToDevice, s));
    }
    HIPCK(h, hipMemsetAsync(err, 0, sizeof(int), s));
    HIPCK(h, launch_gen_primer(s, d_primer, B, P, h->V, h->V, tok, lay.ldtok, err));
    if (P > 0 && g->primer_on_device) {             // a device primer: one check before the token loop
        int e = 0;
        HIPCK(h, hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        if (e) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    if (num == 0) return FSMG_OK;
    HIPCK(h, hipMemsetAsync(hb, 0, sizeof(float) * (size_t)L * 3 * B * Hp, s));

    // position p reads tok[:, p]; primer positions (p < P) run the cells only, generated position t = p - P writes tok[:, p + 1]
    for (int p = 0; p < P + num; ++p) {
        const int pin = p & 1, pout = pin ^ 1;
        const float* x = nullptr;
        for (int l = 0; l < L; ++l) {
            const float* h_in = hb + ((size_t)l * 2 + pin) * B * Hp;
            float* h_out = hb + ((size_t)l * 2 + pout) * B * Hp;
            HIPCK(h, launch_gen_cell(s, h->P + h->off_kx[l], h->in_dim[l], h->P + h->off_kh[l], h->P + h->off_b[l], Hp,
                                     l == 0 ? h->P + h->off_emb : nullptr, h->Ep, tok, lay.ldtok, p, x, h_in, h_out,
                                     cb + (size_t)l * B * Hp, B));
            x = h_out;
        }
        if (p < P) continue;
        HIPCK(h, launch_gen_logits(s, h->P + h->off_w, h->V1p, h->P + h->off_d, h->V1, x, Hp, B, logits, lay.ldl));
        if (!f) {
            HIPCK(h, launch_gen_pick(s, logits, lay.ldl, h->V1, B, g->temperature, g->top_k, g->seed, p - P, tok, lay.ldtok, p + 1, out_tok,
                                     out_lp, num));
        } else {
            const float theta = f->repetition_penalty == 0.f ? 1.f : f->repetition_penalty;
            HIPCK(h, launch_gen_pick_filtered(s, logits, lay.ldl, h->V1, B, g->temperature, g->top_k, f->top_p, f->min_p, theta,
                                              f->repeat_window, g->seed, p - P, tok, lay.ldtok, p + 1, out_tok, out_lp, num));
        }
    }
    const size_t n = (size_t)B * num;
    std::vector<char> host(n * (sizeof(int) + sizeof(float)));
    HIPCK(h, hipMemcpyAsync(host.data(), out_tok, host.size(), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    std::memcpy(out_tokens, host.data(), n * sizeof(int));
    if (out_logprob) std::memcpy(out_logprob, host.data() + n * sizeof(int), n * sizeof(float));
    return FSMG_OK;
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_generate(fsmg_handle h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens, float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, primer, out_tokens, out_logprob);
}

int fsmg_generate_filtered(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* primer, int32_t* out_tokens,
                           float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_gen_config(h, g, primer, out_tokens);
    if (rc == FSMG_OK) rc = check_gen_filters(h, f);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return generate_core(h, g, primer, out_tokens, out_logprob, f);
}

}  // extern "C"
