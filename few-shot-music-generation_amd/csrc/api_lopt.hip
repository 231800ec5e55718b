// Learned optimiser (include/fsmg.h "learned optimiser"): the state, the hooks the MAML-style step, the per-artist driver and
// the outer update call, the entry points.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); every kernel lives in lopt.hip.
#include "fsmg_model.h"
#include "lopt_element.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

static_assert(FSMG_LOPT_NPHI == LOPT_NPHI, "include/fsmg.h and lopt_element.h disagree about Phi");

static int check_lopt_config(fsmg_model* h, const fsmg_lopt_config* c) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_lopt_config");
    if (c->struct_size != (int32_t)sizeof(fsmg_lopt_config))
        return fail(h, FSMG_ERR_INVALID, "fsmg_lopt_config.struct_size is " + std::to_string(c->struct_size) + ", this library expects " +
                                             std::to_string(sizeof(fsmg_lopt_config)));
    if (c->reserved != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_lopt_config.reserved must be zero");
    if (!std::isfinite(c->bF_init) || !std::isfinite(c->bI_init) || !std::isfinite(c->gate_scale) || !std::isfinite(c->phi_lr) || !std::isfinite(c->phi_clip_norm))
        return fail(h, FSMG_ERR_INVALID, "fsmg_lopt_config holds a NaN or a non-finite value");
    if (!(c->gate_scale > 0.f)) return fail(h, FSMG_ERR_INVALID, "gate_scale must be > 0");
    if (!(c->phi_lr >= 0.f)) return fail(h, FSMG_ERR_INVALID, "phi_lr must be >= 0");
    if (!(c->phi_clip_norm >= 0.f)) return fail(h, FSMG_ERR_INVALID, "phi_clip_norm must be >= 0 (0: no clipping)");
    if (c->max_train_steps < 1 || c->max_train_steps > LOPT_MAX_STEPS) return fail(h, FSMG_ERR_INVALID, "max_train_steps must be in [1, 8]");
    return FSMG_OK;
}

static int need_state(fsmg_model* h) {
    return h->lopt_state ? FSMG_OK : fail(h, FSMG_ERR_STATE, "no learned-optimiser state: fsmg_lopt_enable first");
}

// the one allocation, on the first enable: w = 0, the two biases, everything else zero
static int ensure_lopt_state(fsmg_model* h, const fsmg_lopt_config* cfg) {
    if (h->lopt_state) return FSMG_OK;
    const size_t fl = sizeof(float) * (size_t)h->n_flat;
    Carver c;
    const size_t o_phi = c.take(sizeof(float) * 4 * LOPT_NPHI), o_sc = c.take(sizeof(float) * 2 * LOPT_MAX_STEPS), o_fold = c.take(sizeof(double) * LOPT_NPHI),
                 o_part = c.take(sizeof(double) * (size_t)LOPT_MAX_BLOCKS * LOPT_NPHI), o_f = c.take(fl), o_i = c.take(fl);
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (hipMalloc((void**)&h->lopt_state, c.off) != hipSuccess) { h->lopt_state = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(learned-optimiser state) failed"); }
    HIPCK(h, hipMemset(h->lopt_state, 0, c.off));
    h->lopt_phi = (float*)(h->lopt_state + o_phi); h->lopt_pm = h->lopt_phi + LOPT_NPHI; h->lopt_pv = h->lopt_pm + LOPT_NPHI; h->lopt_gphi = h->lopt_pv + LOPT_NPHI;
    h->lopt_sc = (float*)(h->lopt_state + o_sc); h->lopt_fold = (double*)(h->lopt_state + o_fold); h->lopt_part = (double*)(h->lopt_state + o_part);
    h->lopt_F = (float*)(h->lopt_state + o_f); h->lopt_I = (float*)(h->lopt_state + o_i);
    float phi[LOPT_NPHI] = {};
    phi[6] = cfg->bF_init; phi[13] = cfg->bI_init;
    HIPCK(h, hipMemcpy(h->lopt_phi, phi, sizeof(phi), hipMemcpyHostToDevice));
    h->lopt_pending = false;
    return FSMG_OK;
}

// (the caller has drained the stream)
static int ensure_lopt_store(fsmg_model* h, int steps) {
    if (h->lopt_store_steps >= steps) return FSMG_OK;
    if (h->lopt_store) hipFree(h->lopt_store);
    h->lopt_store = nullptr; h->lopt_store_steps = 0;
    const size_t bytes = sizeof(float) * (size_t)h->n_flat * (size_t)steps;
    if (hipMalloc((void**)&h->lopt_store, bytes) != hipSuccess) { h->lopt_store = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(stored support gradients) failed"); }
    HIPCK(h, hipMemset(h->lopt_store, 0, bytes));
    h->lopt_store_steps = steps;
    return FSMG_OK;
}

int lopt_check_train(fsmg_model* h, int inner_steps) {
    if (h->lopt_on && inner_steps > h->lopt_cfg.max_train_steps)
        return fail(h, FSMG_ERR_INVALID, "inner_steps " + std::to_string(inner_steps) + " of a train form exceeds the learned optimiser's max_train_steps " +
                                             std::to_string(h->lopt_cfg.max_train_steps));
    return FSMG_OK;
}

int lopt_begin(fsmg_model* h, bool train) {
    HIPCK(h, launch_fill32(h->stream, h->lopt_F, 0x3f800000u, h->n_flat));         // F_0 = 1.0f
    HIPCK(h, launch_fill32(h->stream, h->lopt_I, 0u, h->n_flat));                  // I_0 = 0
    h->lopt_t = 0;
    h->lopt_storing = train;
    return FSMG_OK;
}

// sgd_update's shape (norm partials, the fused kernel, the K_h images) with the learned rule's kernel
int lopt_inner_update(fsmg_model* h, float lr) {
    hipStream_t s = h->stream;
    const bool slices = h->cfg.clip_norm_mode == FSMG_CLIP_TF1_SLICES;
    const int64_t skip = slices ? round_up((int64_t)h->V1 * h->Ep, FLAT_ALIGN) : 0;
    const int64_t n = h->n_flat - skip;
    const bool store = h->lopt_storing;
    if (store && h->lopt_t >= h->lopt_store_steps) return fail(h, FSMG_ERR_STATE, "more inner steps than the learned optimiser's store holds");
    {
        ScopedTimer tm(h, "update");
        HIPCK(h, launch_sqnorm_partials(s, h->G + skip, n, h->partials));
    }
    LoptUpdateArgs a{};
    a.p = h->P; a.g = h->G; a.F = h->lopt_F; a.I = h->lopt_I; a.phi = h->lopt_phi; a.n = h->n_flat;
    if (store) { a.store = h->lopt_store + (size_t)h->lopt_t * (size_t)h->n_flat; a.sc_step = h->lopt_sc + h->lopt_t; a.sc_loss = h->lopt_sc + LOPT_MAX_STEPS + h->lopt_t; }
    a.partials = h->partials; a.n_partials = sqnorm_blocks(n); a.tail = h->G + h->n_flat; a.use_slices = slices ? 1 : 0;
    a.lr = lr; a.clip = h->cfg.max_grad_norm; a.gate_scale = h->lopt_cfg.gate_scale; a.gnorm_out = h->d_gnorm; a.err_flag = h->d_err;
    {
        ScopedTimer tm(h, store ? "lopt_update_store" : "lopt_update");
        HIPCK(h, launch_lopt_update(s, a));
    }
    ++h->lopt_t;
    h->khf_dirty = true;
    h->have_grads = false;
    return ensure_khf(h);
}

// behind the query pass of a train form, per rank and before any exchange
int lopt_meta_gradient(fsmg_model* h, bool first, double weight) {
    hipStream_t s = h->stream;
    const int K = h->lopt_storing ? h->lopt_t : 0;
    if (K > 0) {
        float* theta_out = nullptr;
        if (h->keep_adapted) {
            if (!h->lopt_replay) {
                HIPCK(h, hipStreamSynchronize(s));
                if (hipMalloc((void**)&h->lopt_replay, sizeof(float) * (size_t)h->n_flat) != hipSuccess) { h->lopt_replay = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(replayed parameters) failed"); }
            }
            theta_out = h->lopt_replay;
            h->lopt_have_replay = true;
        }
        LoptBackpropArgs a{};
        a.G = h->G; a.p0 = h->P_saved; a.store = h->lopt_store; a.stride = h->n_flat; a.sc = h->lopt_sc; a.phi = h->lopt_phi; a.theta_out = theta_out;
        a.n = h->n_flat; a.part = h->lopt_part; a.gate_scale = h->lopt_cfg.gate_scale; a.tail = h->G + h->n_flat; a.err_flag = h->d_err; a.K = K;
        ScopedTimer tm(h, "lopt_backprop");
        HIPCK(h, launch_lopt_backprop(s, a));
    }
    LoptPhiArgs r{};
    r.reduce = 1; r.part = h->lopt_part; r.n_blocks = K > 0 ? lopt_blocks(h->n_flat) : 0; r.weight = weight; r.first = first ? 1 : 0;
    r.fold = h->lopt_fold; r.gphi = h->lopt_gphi;
    {
        ScopedTimer tm(h, "lopt_phi");
        HIPCK(h, launch_lopt_phi(s, r));
    }
    h->lopt_pending = true;
    return FSMG_OK;
}

// inside apply_update, before the launch that counts the step (possibly inside a graph capture: one launch)
int lopt_update_phi(fsmg_model* h, float grad_scale) {
    LoptPhiArgs a{};
    a.reduce = 0; a.gphi = h->lopt_gphi; a.phi = h->lopt_phi; a.m = h->lopt_pm; a.v = h->lopt_pv; a.tail = h->G + h->n_flat; a.err_flag = h->d_err;
    a.grad_scale = grad_scale; a.lr = h->lopt_cfg.phi_lr; a.n_decay = h->cfg.n_decay; a.clip = h->lopt_cfg.phi_clip_norm; a.step = h->d_step;
    ScopedTimer tm(h, "lopt_phi_update");
    HIPCK(h, launch_lopt_phi(h->stream, a));
    return FSMG_OK;
}

static int read14(fsmg_model* h, const float* src, float* host) {
    HIPCK(h, hipMemcpyAsync(host, src, sizeof(float) * LOPT_NPHI, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return FSMG_OK;
}
static int write14(fsmg_model* h, float* dst, const float* host, const char* what) {
    for (int i = 0; i < LOPT_NPHI; ++i)
        if (!std::isfinite(host[i])) return fail(h, FSMG_ERR_INVALID, std::string(what) + " must be finite");
    HIPCK(h, hipStreamSynchronize(h->stream));
    HIPCK(h, hipMemcpy(dst, host, sizeof(float) * LOPT_NPHI, hipMemcpyHostToDevice));
    return FSMG_OK;
}

// fsmg_debug_read's keys of the learned optimiser (api_debug.hip): -1 where `what` is none of them
int lopt_debug_read(fsmg_model* h, const char* what, float* host, int64_t count) {
    if (std::strncmp(what, "lopt_", 5) != 0) return -1;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    if (!std::strcmp(what, "lopt_scalars")) {
        if (count > 2 * LOPT_MAX_STEPS) return fail(h, FSMG_ERR_SIZE, "debug read larger than the buffer");
        HIPCK(h, hipStreamSynchronize(h->stream));
        HIPCK(h, hipMemcpy(host, h->lopt_sc, sizeof(float) * count, hipMemcpyDeviceToHost));
        return FSMG_OK;
    }
    if (!std::strncmp(what, "lopt_F:", 7)) return download_tensor(h, h->lopt_F, what + 7, host, count);
    if (!std::strncmp(what, "lopt_I:", 7)) return download_tensor(h, h->lopt_I, what + 7, host, count);
    if (!std::strncmp(what, "lopt_theta:", 11)) {
        if (!h->lopt_have_replay) return fail(h, FSMG_ERR_STATE, "no replayed parameters kept: fsmg_debug_set(\"keep_adapted\", 1), then a train form with the learned optimiser");
        return download_tensor(h, h->lopt_replay, what + 11, host, count);
    }
    if (!std::strncmp(what, "lopt_g", 6) && what[6] >= '0' && what[6] < '0' + LOPT_MAX_STEPS && what[7] == ':') {
        const int t = what[6] - '0';
        if (t >= h->lopt_store_steps) return fail(h, FSMG_ERR_SIZE, "no such slot in the store");
        return download_tensor(h, h->lopt_store + (size_t)t * (size_t)h->n_flat, what + 8, host, count);
    }
    return fail(h, FSMG_ERR_NAME, std::string("unknown debug buffer '") + what + "'");
}

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_lopt_enable(fsmg_handle h, const fsmg_lopt_config* cfg) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_lopt_config(h, cfg);
    if (rc != FSMG_OK) return rc;
    if (h->comm) return fail(h, FSMG_ERR_STATE, "a communicator is attached: the library's exchange does not carry GPhi");
    if (h->msgd_on) return fail(h, FSMG_ERR_STATE, "Meta-SGD is enabled on this handle (fsmg_msgd_disable first)");
    BEGIN_CALL(h);
    if ((rc = ensure_lopt_state(h, cfg)) != FSMG_OK) return rc;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->aux) HIPCK(h, hipStreamSynchronize(h->aux));
    if ((rc = ensure_lopt_store(h, cfg->max_train_steps)) != FSMG_OK) return rc;
    drop_graphs(h);                     // (a captured update holds the scalars of the configuration it was captured under)
    h->lopt_cfg = *cfg;
    h->lopt_on = true;
    h->lopt_pending = false;
    return FSMG_OK;
}

int fsmg_lopt_disable(fsmg_handle h) {
    if (!h) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    h->lopt_on = false;
    h->lopt_pending = false;
    return FSMG_OK;
}

int fsmg_lopt_info(fsmg_handle h, int64_t out[4]) {
    if (!h || !out) return FSMG_ERR_INVALID;
    out[0] = h->lopt_on ? 1 : 0; out[1] = h->lopt_state ? 1 : 0; out[2] = h->lopt_state ? h->lopt_cfg.max_train_steps : 0;
    out[3] = (h->lopt_on && h->lopt_pending && h->have_grads) ? 1 : 0;
    return FSMG_OK;
}

int fsmg_lopt_get_phi(fsmg_handle h, float* phi) {
    if (!h || !phi) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return read14(h, h->lopt_phi, phi);
}

int fsmg_lopt_set_phi(fsmg_handle h, const float* phi) {
    if (!h || !phi) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return write14(h, h->lopt_phi, phi, "a weight of Phi");
}

int fsmg_lopt_get_opt_state(fsmg_handle h, float* m, float* v) {
    if (!h || !m || !v) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    rc = read14(h, h->lopt_pm, m);
    return rc != FSMG_OK ? rc : read14(h, h->lopt_pv, v);
}

int fsmg_lopt_set_opt_state(fsmg_handle h, const float* m, const float* v) {
    if (!h || !m || !v) return FSMG_ERR_INVALID;
    int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    rc = write14(h, h->lopt_pm, m, "an Adam slot of Phi");
    return rc != FSMG_OK ? rc : write14(h, h->lopt_pv, v, "an Adam slot of Phi");
}

int fsmg_lopt_get_grad(fsmg_handle h, float* gphi) {
    if (!h || !gphi) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    if (!(h->lopt_on && h->lopt_pending && h->have_grads))
        return fail(h, FSMG_ERR_STATE, "no GPhi is pending: a train form of fsmg_maml_* on an enabled handle first");
    BEGIN_CALL(h);
    return read14(h, h->lopt_gphi, gphi);
}

int fsmg_lopt_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count) {
    if (!h || !device_ptr || !count) return FSMG_ERR_INVALID;
    const int rc = need_state(h);
    if (rc != FSMG_OK) return rc;
    *device_ptr = h->lopt_gphi;
    *count = LOPT_NPHI;
    return FSMG_OK;
}

}  // extern "C"
