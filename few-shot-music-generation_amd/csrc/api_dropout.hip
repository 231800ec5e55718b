// Dropout of the train passes (include/fsmg.h "Dropout"): the switch, the pass counter, the masked copies, the hooks
// forward() / backward() call, the entry points.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); every kernel lives in dropout.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

static bool keep_ok(float k) { return k > 0.0f && k <= 1.0f; }      // (a NaN fails both)

static int check_dropout_config(fsmg_model* h, const fsmg_dropout_config* c) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_dropout_config");
    if (c->struct_size != (int32_t)sizeof(fsmg_dropout_config))
        return fail(h, FSMG_ERR_INVALID, "fsmg_dropout_config.struct_size is " + std::to_string(c->struct_size) + ", this library expects " +
                                             std::to_string(sizeof(fsmg_dropout_config)));
    if (!keep_ok(c->keep_input)) return fail(h, FSMG_ERR_INVALID, "keep_input must be in (0, 1]");
    if (!keep_ok(c->keep_output)) return fail(h, FSMG_ERR_INVALID, "keep_output must be in (0, 1]");
    if (c->variational != 0 && c->variational != 1) return fail(h, FSMG_ERR_INVALID, "variational must be 0 or 1");
    return FSMG_OK;
}

// the arguments of one site for a pass of B sequences with the handle's scalars
static DropArgs site_args(const fsmg_model* h, uint32_t pass, int site, int B) {
    const float keep = drop_keep(h, site);
    DropArgs a{};
    a.key0 = (uint32_t)(h->drop_cfg.seed & 0xffffffffull); a.key1 = (uint32_t)(h->drop_cfg.seed >> 32);
    a.site = (uint32_t)site; a.pass = pass;
    a.thr = (uint32_t)(keep * 16777216.0f);             // truncation; keep == 1: 2^24, above every 24-bit word
    a.scale = 1.0f / keep;
    a.variational = h->drop_cfg.variational; a.B = B;
    a.W = site == 0 ? h->E : h->H; a.ld = site == 0 ? h->Ep : h->Hp;
    a.rows = (long long)h->T * B;
    return a;
}

// the masked copies hold B sequences: one allocation, grown (after a stream sync) when a pass brings more rows than any before
static int ensure_drop_copies(fsmg_model* h, int B) {
    if (h->drop_state != nullptr && h->drop_cap >= B) return FSMG_OK;
    const int cap = std::max(B, h->Bcap);
    Carver c;
    std::vector<size_t> off((size_t)h->L + 1);
    for (int s = 0; s <= h->L; ++s) off[(size_t)s] = c.take(sizeof(float) * (size_t)h->T * cap * (s == 0 ? h->Ep : h->Hp));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->aux) HIPCK(h, hipStreamSynchronize(h->aux));
    drop_destroy(h);
    if (hipMalloc((void**)&h->drop_state, c.off) != hipSuccess) { h->drop_state = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(dropout copies) failed"); }
    h->drop_cap = cap; h->drop_bytes = (int64_t)c.off;
    h->drop_buf.assign((size_t)h->L + 1, nullptr);
    h->drop_lastB.assign((size_t)h->L + 1, 0);
    for (int s = 0; s <= h->L; ++s) h->drop_buf[(size_t)s] = (float*)(h->drop_state + off[(size_t)s]);
    return FSMG_OK;
}

void drop_destroy(fsmg_model* h) {
    if (h->drop_state) hipFree(h->drop_state);
    h->drop_state = nullptr; h->drop_cap = 0; h->drop_bytes = 0;
    h->drop_buf.clear(); h->drop_lastB.clear();
}

int drop_begin_pass(fsmg_model* h, int B) {
    h->drop_call = h->drop_on && !h->drop_suppress;
    if (!h->drop_call) return FSMG_OK;
    const int rc = ensure_drop_copies(h, B);
    if (rc != FSMG_OK) h->drop_call = false;
    return rc;
}

void drop_take_index(fsmg_model* h) {
    if (!h->drop_call) return;
    h->drop_last = (int64_t)h->drop_next;
    h->drop_pass = (uint32_t)(h->drop_next & 0xffffffffull);
    ++h->drop_next;
}

int drop_forward_site(fsmg_model* h, int site, int B) {
    if (!drop_site_on(h, site)) return FSMG_OK;
    const DropArgs a = site_args(h, h->drop_pass, site, B);
    if (B > h->drop_cap) return fail(h, FSMG_ERR_STATE, "internal: dropped pass over more sequences than the masked copies hold");
    if (site == 0) {
        ScopedTimer tm(h, "dropout_embed_fwd");
        HIPCK(h, launch_dropout_embed_fwd(h->stream, a, h->P + h->off_emb, h->X, h->drop_buf[0]));
    } else {
        ScopedTimer tm(h, "dropout_fwd");
        HIPCK(h, launch_dropout_fwd(h->stream, a, h->Hs[site - 1] + (size_t)B * h->Hp, h->drop_buf[(size_t)site]));
    }
    h->drop_lastB[(size_t)site] = B;
    return FSMG_OK;
}

int drop_backward_site(fsmg_model* h, int site, int B, float* g) {
    if (!drop_site_on(h, site)) return FSMG_OK;
    ScopedTimer tm(h, site == 0 ? "dropout_bwd_emb" : "dropout_bwd");        // (two classes: the rows differ in width, tools/dropout_bench.py)
    HIPCK(h, launch_dropout_bwd(h->stream, site_args(h, h->drop_pass, site, B), g));
    return FSMG_OK;
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_dropout_enable(fsmg_handle h, const fsmg_dropout_config* cfg) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_dropout_config(h, cfg);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    if ((rc = ensure_drop_copies(h, std::max(1, h->Bcap))) != FSMG_OK) return rc;
    h->drop_cfg = *cfg;
    h->drop_on = true; h->drop_ever = true;
    return FSMG_OK;
}

int fsmg_dropout_disable(fsmg_handle h) {
    if (!h) return FSMG_ERR_INVALID;
    h->drop_on = false;
    return FSMG_OK;
}

int fsmg_dropout_info(fsmg_handle h, int64_t out[4]) {
    if (!h || !out) return FSMG_ERR_INVALID;
    out[0] = h->drop_on ? 1 : 0; out[1] = h->drop_last; out[2] = (int64_t)h->drop_next; out[3] = h->drop_bytes;
    return FSMG_OK;
}

int fsmg_dropout_set_pass(fsmg_handle h, int64_t next_pass) {
    if (!h) return FSMG_ERR_INVALID;
    if (next_pass < 0) return fail(h, FSMG_ERR_INVALID, "next_pass must be >= 0");
    if (!h->drop_ever) return fail(h, FSMG_ERR_STATE, "no dropout scalars: fsmg_dropout_enable first");
    h->drop_next = (uint64_t)next_pass;
    return FSMG_OK;
}

int fsmg_dropout_mask(fsmg_handle h, int64_t pass, int32_t site, int32_t B, uint8_t* out) {
    if (!h || !out) return FSMG_ERR_INVALID;
    if (pass < 0 || site < 0 || site > h->L || B < 1 || (int64_t)B * h->T > (1 << 24)) return fail(h, FSMG_ERR_INVALID, "bad pass / site / B");
    if (!h->drop_ever) return fail(h, FSMG_ERR_STATE, "no dropout scalars: fsmg_dropout_enable first");
    BEGIN_CALL(h);
    const DropArgs a = site_args(h, (uint32_t)((uint64_t)pass & 0xffffffffull), site, B);
    const size_t bytes = (size_t)a.rows * a.W;
    unsigned char* d = nullptr;
    if (hipMalloc((void**)&d, bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(mask bytes) failed");
    hipError_t e = launch_dropout_mask(h->stream, a, d);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(h, FSMG_ERR_HIP, std::string("fsmg_dropout_mask: ") + hipGetErrorString(e));
    return FSMG_OK;
}

}  // extern "C"
