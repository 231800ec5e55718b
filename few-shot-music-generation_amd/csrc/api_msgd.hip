// Meta-SGD (include/fsmg.h "Meta-SGD"): the rates' state, the hooks the MAML-style step and the outer update call, the
// entry points.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); every kernel lives in msgd.hip / elementwise.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

static uint32_t float_bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

static int check_msgd_config(fsmg_model* h, const fsmg_msgd_config* c) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_msgd_config");
    if (c->struct_size != (int32_t)sizeof(fsmg_msgd_config))
        return fail(h, FSMG_ERR_INVALID, "fsmg_msgd_config.struct_size is " + std::to_string(c->struct_size) + ", this library expects " +
                                             std::to_string(sizeof(fsmg_msgd_config)));
    if (c->reserved != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_msgd_config.reserved must be zero");
    if (std::isnan(c->alpha_init) || std::isnan(c->alpha_lr) || std::isnan(c->alpha_min) || std::isnan(c->alpha_max) || std::isnan(c->alpha_clip_norm))
        return fail(h, FSMG_ERR_INVALID, "fsmg_msgd_config holds a NaN");
    if (!std::isfinite(c->alpha_init)) return fail(h, FSMG_ERR_INVALID, "alpha_init must be finite");
    if (!(c->alpha_lr >= 0.f) || !std::isfinite(c->alpha_lr)) return fail(h, FSMG_ERR_INVALID, "alpha_lr must be finite and >= 0");
    if (!(c->alpha_clip_norm >= 0.f) || !std::isfinite(c->alpha_clip_norm)) return fail(h, FSMG_ERR_INVALID, "alpha_clip_norm must be finite and >= 0 (0: no clipping)");
    if (c->alpha_min > c->alpha_max) return fail(h, FSMG_ERR_INVALID, "alpha_min must not exceed alpha_max");
    return FSMG_OK;
}

static int need_state(fsmg_model* h) {
    return h->msgd_state ? FSMG_OK : fail(h, FSMG_ERR_STATE, "no Meta-SGD state: fsmg_msgd_enable first");
}

// A = value, slots zero (stream order)
static int fill_rates(fsmg_model* h, float value) {
    HIPCK(h, launch_fill32(h->stream, h->msgd_A, float_bits(value), h->n_flat));
    HIPCK(h, launch_fill32(h->stream, h->msgd_AM, 0u, 2 * h->n_flat));            // AM and AV are adjacent
    return FSMG_OK;
}

// the one allocation, on the first enable: A = alpha_init, everything else zero
static int ensure_msgd_state(fsmg_model* h, float alpha_init) {
    if (h->msgd_state) return FSMG_OK;
    const size_t fl = sizeof(float) * (size_t)h->n_flat;
    Carver c;
    const size_t o_a = c.take(fl), o_m = c.take(2 * fl), o_s = c.take(fl), o_g = c.take(fl),
                 o_p = c.take(sizeof(double) * (size_t)sqnorm_blocks(h->n_flat));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (hipMalloc((void**)&h->msgd_state, c.off) != hipSuccess) { h->msgd_state = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(Meta-SGD state) failed"); }
    HIPCK(h, hipMemset(h->msgd_state, 0, c.off));
    h->msgd_A = (float*)(h->msgd_state + o_a); h->msgd_AM = (float*)(h->msgd_state + o_m); h->msgd_AV = h->msgd_AM + h->n_flat;
    h->msgd_S = (float*)(h->msgd_state + o_s); h->msgd_GA = (float*)(h->msgd_state + o_g); h->msgd_part = (double*)(h->msgd_state + o_p);
    h->msgd_pending = false;
    return fill_rates(h, alpha_init);
}

int msgd_begin_sum(fsmg_model* h) {
    HIPCK(h, launch_fill32(h->stream, h->msgd_S, 0u, h->n_flat));
    return FSMG_OK;
}

// sgd_update's shape (norm partials, the fused kernel, the K_h images) with the rates' kernel
int msgd_inner_update(fsmg_model* h, float lr, bool with_sum) {
    hipStream_t s = h->stream;
    const bool slices = h->cfg.clip_norm_mode == FSMG_CLIP_TF1_SLICES;
    const int64_t skip = slices ? round_up((int64_t)h->V1 * h->Ep, FLAT_ALIGN) : 0;
    const int64_t n = h->n_flat - skip;
    {
        ScopedTimer tm(h, "update");
        HIPCK(h, launch_sqnorm_partials(s, h->G + skip, n, h->partials));
    }
    MsgdUpdateArgs a{};
    a.p = h->P; a.g = h->G; a.alpha = h->msgd_A; a.sum = with_sum ? h->msgd_S : nullptr; a.n = h->n_flat;
    a.partials = h->partials; a.n_partials = sqnorm_blocks(n); a.tail = h->G + h->n_flat; a.use_slices = slices ? 1 : 0;
    a.lr = lr; a.clip = h->cfg.max_grad_norm; a.gnorm_out = h->d_gnorm; a.err_flag = h->d_err;
    {
        ScopedTimer tm(h, with_sum ? "msgd_update_sum" : "msgd_update");
        HIPCK(h, launch_msgd_update(s, a));
    }
    h->khf_dirty = true;
    h->have_grads = false;
    return ensure_khf(h);
}

// behind the query pass of a train form, per rank and before any exchange
int msgd_rate_gradient(fsmg_model* h) {
    {
        ScopedTimer tm(h, "msgd_alpha_grad");
        HIPCK(h, launch_msgd_alpha_grad(h->stream, h->msgd_GA, h->G, h->msgd_S, h->n_flat));
    }
    h->msgd_pending = true;
    return FSMG_OK;
}

// inside apply_update, before the launch that counts the step (possibly inside a graph capture: launches only)
int msgd_update_rates(fsmg_model* h, float grad_scale) {
    hipStream_t s = h->stream;
    HIPCK(h, launch_sqnorm_partials(s, h->msgd_GA, h->n_flat, h->msgd_part));
    MsgdAlphaArgs a{};
    a.alpha = h->msgd_A; a.m = h->msgd_AM; a.v = h->msgd_AV; a.ga = h->msgd_GA; a.n = h->n_flat;
    a.partials = h->msgd_part; a.n_partials = sqnorm_blocks(h->n_flat); a.tail = h->G + h->n_flat; a.err_flag = h->d_err;
    a.grad_scale = grad_scale; a.lr = h->msgd_cfg.alpha_lr; a.n_decay = h->cfg.n_decay; a.clip = h->msgd_cfg.alpha_clip_norm;
    a.lo = h->msgd_cfg.alpha_min; a.hi = h->msgd_cfg.alpha_max; a.step = h->d_step;
    ScopedTimer tm(h, "msgd_alpha_update");
    HIPCK(h, launch_msgd_alpha_update(s, a));
    return FSMG_OK;
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_msgd_enable(fsmg_handle h, const fsmg_msgd_config* cfg) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_msgd_config(h, cfg);
    if (rc != FSMG_OK) return rc;
    if (h->comm) return fail(h, FSMG_ERR_STATE, "a communicator is attached: the library's exchange does not carry the rate gradient");
    if (h->lopt_on) return fail(h, FSMG_ERR_STATE, "the learned optimiser is enabled on this handle (fsmg_lopt_disable first)");
    BEGIN_CALL(h);
    if ((rc = ensure_msgd_state(h, cfg->alpha_init)) != FSMG_OK) return rc;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->aux) HIPCK(h, hipStreamSynchronize(h->aux));
    drop_graphs(h);                     // (a captured update holds the scalars of the configuration it was captured under)
    h->msgd_cfg = *cfg;
    h->msgd_on = true;
    return FSMG_OK;
}

int fsmg_msgd_disable(fsmg_handle h) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    h->msgd_on = false;
    h->msgd_pending = false;
    return FSMG_OK;
}

int fsmg_msgd_info(fsmg_handle h, int64_t out[4]) {
    if (!h || !out) return FSMG_ERR_INVALID;
    out[0] = h->msgd_on ? 1 : 0; out[1] = h->msgd_state ? 1 : 0; out[2] = h->n_flat;
    out[3] = (h->msgd_on && h->msgd_pending && h->have_grads) ? 1 : 0;
    return FSMG_OK;
}

int fsmg_msgd_fill(fsmg_handle h, float value) {
    if (!h) return FSMG_ERR_INVALID;
    if (!std::isfinite(value)) return fail(h, FSMG_ERR_INVALID, "a rate must be finite");
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return fill_rates(h, value);
}

int fsmg_msgd_get_alpha(fsmg_handle h, const char* name, float* host, int64_t count) {
    if (!h || !name || !host) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return download_tensor(h, h->msgd_A, name, host, count);
}

int fsmg_msgd_set_alpha(fsmg_handle h, const char* name, const float* host, int64_t count) {
    if (!h || !name || !host) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    const ParamDesc* p = find_param(h, name);
    if (!p) return fail(h, FSMG_ERR_NAME, std::string("unknown parameter '") + name + "'");
    if (count != p->rows * p->cols) return fail(h, FSMG_ERR_SIZE, std::string("size mismatch for '") + name + "'");
    for (int64_t i = 0; i < count; ++i)
        if (!std::isfinite(host[i])) return fail(h, FSMG_ERR_INVALID, "a rate must be finite");
    BEGIN_CALL(h);
    return upload_tensor(h, h->msgd_A, name, host, count);
}

int fsmg_msgd_get_opt_state(fsmg_handle h, const char* name, float* m, float* v, int64_t count) {
    if (!h || !name || !m || !v) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    rc = download_tensor(h, h->msgd_AM, name, m, count);
    return rc != FSMG_OK ? rc : download_tensor(h, h->msgd_AV, name, v, count);
}

int fsmg_msgd_set_opt_state(fsmg_handle h, const char* name, const float* m, const float* v, int64_t count) {
    if (!h || !name || !m || !v) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    rc = upload_tensor(h, h->msgd_AM, name, m, count);
    return rc != FSMG_OK ? rc : upload_tensor(h, h->msgd_AV, name, v, count);
}

int fsmg_msgd_get_grad(fsmg_handle h, const char* name, float* host, int64_t count) {
    if (!h || !name || !host) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    if (!(h->msgd_on && h->msgd_pending && h->have_grads))
        return fail(h, FSMG_ERR_STATE, "no rate gradient is pending: fsmg_maml_forward_backward* on an enabled handle first");
    BEGIN_CALL(h);
    return download_tensor(h, h->msgd_GA, name, host, count);
}

int fsmg_msgd_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count) {
    if (!h || !device_ptr || !count) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    *device_ptr = h->msgd_GA;
    *count = h->n_flat;
    return FSMG_OK;
}

}  // extern "C"
