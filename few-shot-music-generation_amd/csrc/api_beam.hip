// Batched on-device beam search (fsmg_beam_search; fsmg_maml_beam_search lives beside fsmg_maml_generate in api_step.hip).
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in decode.hip.  DESIGN.md "Beam search".
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

namespace {
constexpr size_t BEAM_ALIGN = 256;
size_t beam_align(size_t n) { return (n + BEAM_ALIGN - 1) / BEAM_ALIGN * BEAM_ALIGN; }

// one call's scratch in h->gen (R = G * W rows): h and c twice ([L][R][Hp] each: the cells' ping-pong / the reorder's target), the
// logits rows, the token buffer [R][P+num+1], cum [R], the candidates [R][W], the per-position parent / token / lp [num][R], the
// outputs (tokens, lps, scores: one contiguous D2H copy), a staged host primer, the primer error flag
struct BeamLayout {
    size_t h0, h1, c0, c1, logits, tok, cum, cand_s, cand_lp, cand_v, par, htok, hlp, out_tok, out_lp, out_score, primer, err, total;
    int ldl, ldtok;
};
BeamLayout beam_layout(const fsmg_model* h, int G, int W, int P, int num) {
    BeamLayout b{};
    const size_t R = (size_t)G * W, state = sizeof(float) * (size_t)h->L * R * h->Hp;
    b.ldl = (int)round_up(h->V1, 64);
    b.ldtok = P + num + 1;
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off += beam_align(bytes); return o; };
    b.h0 = place(state);
    b.h1 = place(state);
    b.c0 = place(state);
    b.c1 = place(state);
    b.logits = place(sizeof(float) * R * b.ldl);
    b.tok = place(sizeof(int) * R * b.ldtok);
    b.cum = place(sizeof(float) * R);
    b.cand_s = place(sizeof(float) * R * W);
    b.cand_lp = place(sizeof(float) * R * W);
    b.cand_v = place(sizeof(int) * R * W);
    b.par = place(sizeof(int) * (size_t)num * R);
    b.htok = place(sizeof(int) * (size_t)num * R);
    b.hlp = place(sizeof(float) * (size_t)num * R);
    b.out_tok = off;                                       // out_tok, out_lp and out_score back to back: one copy
    off += sizeof(int) * R * num;
    b.out_lp = off;
    off += sizeof(float) * R * num;
    b.out_score = off;
    off = beam_align(off + sizeof(float) * R);
    b.primer = place(sizeof(int) * (size_t)G * P);
    b.err = place(sizeof(int));
    b.total = off;
    return b;
}
}  // namespace

int check_beam_config(fsmg_model* h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores) {
    if (!b) return fail(h, FSMG_ERR_INVALID, "null fsmg_beam_config");
    if (b->version != FSMG_BEAM_CONFIG_VERSION)
        return fail(h, FSMG_ERR_INVALID, "fsmg_beam_config.version is " + std::to_string(b->version) + ", this library expects " +
                                             std::to_string(FSMG_BEAM_CONFIG_VERSION));
    for (int i = 0; i < 8; ++i)
        if (b->reserved[i] != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_beam_config.reserved must be zero");
    if (b->n_groups < 1 || b->num < 1 || b->primer_len < 0) return fail(h, FSMG_ERR_INVALID, "n_groups and num must be >= 1, primer_len >= 0");
    if (b->beam_width < 1 || b->beam_width > 64) return fail(h, FSMG_ERR_INVALID, "beam_width must be in [1, 64]");
    int64_t seqs = 1;                               // V1^num, stopped once it reaches W (no overflow)
    for (int t = 0; t < b->num && seqs < b->beam_width; ++t) seqs *= h->V1;
    if (seqs < b->beam_width) return fail(h, FSMG_ERR_INVALID, "beam_width exceeds the (input_size + 1)^num distinct sequences");
    if (b->primer_on_device != 0 && b->primer_on_device != 1) return fail(h, FSMG_ERR_INVALID, "primer_on_device must be 0 or 1");
    if (b->primer_len > 0 && !primer) return fail(h, FSMG_ERR_INVALID, "primer_len > 0 needs a primer");
    if (!out_tokens || !out_scores) return fail(h, FSMG_ERR_INVALID, "null out_tokens / out_scores");
    // (as check_gen_config: the cells' grid y dimension and 32-bit token offsets, over the G * W rows)
    const int64_t R = (int64_t)b->n_groups * b->beam_width;
    if (R > (1 << 20) || R * ((int64_t)b->primer_len + b->num + 1) > (1LL << 30))
        return fail(h, FSMG_ERR_INVALID, "n_groups * beam_width * (primer_len + num + 1) too large");
    return FSMG_OK;
}

int beam_core(fsmg_model* h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob) {
    const int G = b->n_groups, W = b->beam_width, R = G * W, P = b->primer_len, num = b->num, L = h->L, Hp = h->Hp;
    if (P > 0 && !b->primer_on_device) {           // a host primer is checked before any device work
        for (int64_t i = 0; i < (int64_t)G * P; ++i)
            if (primer[i] < 0 || primer[i] >= h->V) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    hipStream_t s = h->stream;
    const BeamLayout lay = beam_layout(h, G, W, P, num);
    const int rc = gen_reserve(h, lay.total);
    if (rc != FSMG_OK) return rc;
    char* base = h->gen;
    float* h_in = (float*)(base + lay.h0);         // [L][R][Hp]: the cells read h_in and write h_out
    float* h_out = (float*)(base + lay.h1);
    float* c = (float*)(base + lay.c0);            // [L][R][Hp]: updated in place by the cells, gathered into c_spare
    float* c_spare = (float*)(base + lay.c1);
    float* logits = (float*)(base + lay.logits);
    int* tok = (int*)(base + lay.tok);
    float* cum = (float*)(base + lay.cum);
    float* cand_s = (float*)(base + lay.cand_s);
    float* cand_lp = (float*)(base + lay.cand_lp);
    int* cand_v = (int*)(base + lay.cand_v);
    int* par = (int*)(base + lay.par);
    int* htok = (int*)(base + lay.htok);
    float* hlp = (float*)(base + lay.hlp);
    int* err = (int*)(base + lay.err);
    const size_t layer = (size_t)R * Hp;

    const int32_t* d_primer = primer;
    if (P > 0 && !b->primer_on_device) {
        d_primer = (const int32_t*)(base + lay.primer);
        HIPCK(h, hipMemcpyAsync((void*)d_primer, primer, sizeof(int) * (size_t)G * P, hipMemcpyHostToDevice, s));
    }
    HIPCK(h, hipMemsetAsync(err, 0, sizeof(int), s));
    // the primer runs on all G * W rows (row r reads primer[r / W]): the slots of a group stay identical until the first pick
    HIPCK(h, launch_gen_primer(s, d_primer, R, P, h->V, h->V, tok, lay.ldtok, err, W));
    if (P > 0 && b->primer_on_device) {             // a device primer: one check before the token loop
        int e = 0;
        HIPCK(h, hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        if (e) return fail(h, FSMG_ERR_TOKEN_RANGE, "primer id outside [0, input_size)");
    }
    HIPCK(h, hipMemsetAsync(h_in, 0, sizeof(float) * L * layer, s));
    HIPCK(h, hipMemsetAsync(c, 0, sizeof(float) * L * layer, s));
    HIPCK(h, launch_beam_init(s, cum, R, W));

    // position p reads tok[:, p]; generated position t = p - P writes tok[:, p + 1] and par / htok / hlp [t]
    for (int p = 0; p < P + num; ++p) {
        const float* x = nullptr;
        for (int l = 0; l < L; ++l) {
            HIPCK(h, launch_gen_cell(s, h->P + h->off_kx[l], h->in_dim[l], h->P + h->off_kh[l], h->P + h->off_b[l], Hp,
                                     l == 0 ? h->P + h->off_emb : nullptr, h->Ep, tok, lay.ldtok, p, x, h_in + l * layer, h_out + l * layer,
                                     c + l * layer, R));
            x = h_out + l * layer;
        }
        if (p < P) {                                // no choice yet: the new state is every row's own
            std::swap(h_in, h_out);
            continue;
        }
        const int t = p - P;
        HIPCK(h, launch_gen_logits(s, h->P + h->off_w, h->V1p, h->P + h->off_d, h->V1, x, Hp, R, logits, lay.ldl));
        HIPCK(h, launch_beam_rowtop(s, logits, lay.ldl, h->V1, R, W, cum, cand_s, cand_lp, cand_v));
        HIPCK(h, launch_beam_select(s, G, W, h->V1, cand_s, cand_lp, cand_v, cum, tok, lay.ldtok, p + 1, par + (size_t)t * R,
                                    htok + (size_t)t * R, hlp + (size_t)t * R));
        if (t + 1 < num) {                          // each slot continues from its parent's state
            HIPCK(h, launch_beam_reorder(s, L, R, W, Hp, par + (size_t)t * R, h_out, h_in, c, c_spare));
            std::swap(c, c_spare);
        }
    }
    int* out_tok = (int*)(base + lay.out_tok);
    float* out_lp = (float*)(base + lay.out_lp);
    float* out_sc = (float*)(base + lay.out_score);
    HIPCK(h, launch_beam_backtrace(s, R, W, num, par, htok, hlp, cum, out_tok, out_lp, out_sc));
    const size_t n = (size_t)R * num;
    std::vector<char> host(n * (sizeof(int) + sizeof(float)) + sizeof(float) * R);
    HIPCK(h, hipMemcpyAsync(host.data(), out_tok, host.size(), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    std::memcpy(out_tokens, host.data(), n * sizeof(int));
    if (out_logprob) std::memcpy(out_logprob, host.data() + n * sizeof(int), n * sizeof(float));
    std::memcpy(out_scores, host.data() + n * (sizeof(int) + sizeof(float)), sizeof(float) * R);
    return FSMG_OK;
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_beam_search(fsmg_handle h, const fsmg_beam_config* b, const int32_t* primer, int32_t* out_tokens, float* out_scores,
                     float* out_logprob) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_beam_config(h, b, primer, out_tokens, out_scores);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return beam_core(h, b, primer, out_tokens, out_scores, out_logprob);
}

}  // extern "C"
