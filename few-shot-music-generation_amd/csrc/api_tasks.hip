// Per-artist MAML (include/fsmg.h "per-artist MAML"): the episode as a meta-batch of N tasks.  The driver loops over the
// artists around the adaptation and the query pass of the fsmg_maml_* entry points as they stand (api_step.hip) and folds behind each.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the fold's kernel lives in tasks.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace {

// where the call's rows are once the arguments are checked (and, for the table form, gathered): artist n's support rows start at
// sup + n * K * T, its lengths at slen + n * K
struct Episode {
    const int32_t *sup = nullptr, *qry = nullptr, *slen = nullptr, *qlen = nullptr;
    int on_device = 0;
    bool masked = false;
};

// every argument error of the three entry points, before any device work
int check_tasks_args(fsmg_model* h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query, const int32_t* support_len,
                     const int32_t* query_len, int32_t N, int32_t K, int32_t Q) {
    if (!c) return fail(h, FSMG_ERR_INVALID, "null fsmg_maml_tasks_config");
    if (c->struct_size != (int32_t)sizeof(fsmg_maml_tasks_config))
        return fail(h, FSMG_ERR_INVALID, "fsmg_maml_tasks_config.struct_size is " + std::to_string(c->struct_size) + ", this library expects " +
                                             std::to_string(sizeof(fsmg_maml_tasks_config)));
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return fail(h, FSMG_ERR_INVALID, "fsmg_maml_tasks_config.reserved must be zero");
    if (!support || !query) return fail(h, FSMG_ERR_INVALID, "null token pointer");
    if (c->inner_steps < 0 || c->inner_steps > 64 || !(c->inner_lr >= 0.f) || K <= 0 || Q <= 0)
        return fail(h, FSMG_ERR_INVALID, "bad inner_steps / inner_lr / K / Q");
    if (c->tokens_on_device != 0 && c->tokens_on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (c->table_id < -1 || c->table_id >= fsmg_model::MAX_TABLES) return fail(h, FSMG_ERR_INVALID, "table_id outside [-1, 4)");
    if (c->use_table_lengths != 0 && c->use_table_lengths != 1) return fail(h, FSMG_ERR_INVALID, "use_table_lengths must be 0 or 1");
    if (c->table_id < 0 && c->use_table_lengths) return fail(h, FSMG_ERR_INVALID, "use_table_lengths needs a table_id");
    if ((support_len == nullptr) != (query_len == nullptr)) return fail(h, FSMG_ERR_INVALID, "support_len and query_len go together");
    if (c->table_id >= 0 && support_len) return fail(h, FSMG_ERR_INVALID, "a table call takes the table's lengths (use_table_lengths), not length pointers");
    int rc = validate_shape(h, N, K, Q);
    if (rc != FSMG_OK) return rc;
    if (support_len) rc = validate_masked_args(h, support_len, query_len, N, K, Q, c->tokens_on_device);
    return rc;
}

// the table form gathers the episode's rows (and lengths) once; the token form is where the caller says
int locate_episode(fsmg_model* h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query, const int32_t* support_len,
                   const int32_t* query_len, int32_t N, int32_t K, int32_t Q, Episode* e) {
    if (c->table_id < 0) {
        e->sup = support; e->qry = query; e->slen = support_len; e->qlen = query_len;
        e->on_device = c->tokens_on_device; e->masked = support_len != nullptr;
        return FSMG_OK;
    }
    e->masked = c->use_table_lengths != 0;
    const int rc = gather_episode_rows(h, c->table_id, support, N * K, query, N * Q, e->masked);
    if (rc != FSMG_OK) return rc;
    e->sup = h->d_gather; e->qry = h->d_gather + (size_t)N * K * h->T; e->on_device = 1;
    if (e->masked) { e->slen = h->d_gather_len; e->qlen = h->d_gather_len + (size_t)N * K; }
    return FSMG_OK;
}

// ACC and d_task_loss: allocated on first use, kept until fsmg_destroy
int ensure_task_buffers(fsmg_model* h, int N) {
    if (h->task_acc && h->task_loss_cap >= N) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (!h->task_acc) {
        const size_t bytes = sizeof(float) * (size_t)(h->n_flat + FSMG_GRAD_TAIL);
        if (hipMalloc((void**)&h->task_acc, bytes) != hipSuccess) { h->task_acc = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(per-artist gradient fold) failed"); }
        HIPCK(h, hipMemset(h->task_acc, 0, bytes));
    }
    if (h->task_loss_cap < N) {
        if (h->d_task_loss) hipFree(h->d_task_loss);
        h->d_task_loss = nullptr; h->task_loss_cap = 0;
        const int cap = std::max(N, 64);
        if (hipMalloc((void**)&h->d_task_loss, sizeof(float) * (size_t)cap) != hipSuccess) { h->d_task_loss = nullptr; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(per-artist losses) failed"); }
        h->task_loss_cap = cap;
    }
    return FSMG_OK;
}

// behind artist n's query pass: the fold, theta back, the recurrent-weight images rebuilt as restore_theta rebuilds them
int fold_artist(fsmg_model* h, int n, int N) {
    TaskFoldArgs a{};
    a.g = h->G; a.acc = h->task_acc; a.p = h->P; a.p_saved = h->P_saved; a.n = h->n_flat;
    if (h->msgd_on) { a.s = h->msgd_S; a.ga = h->msgd_GA; }
    a.w = (float)(1.0 / (double)N); a.first = n == 0; a.last = n == N - 1; a.task_loss = h->d_task_loss + n;
    {
        ScopedTimer tm(h, "task_fold");
        HIPCK(h, launch_task_fold(h->stream, a));
    }
    h->khf_dirty = true;
    return ensure_khf(h);
}

int tasks_forward_backward(fsmg_model* h, const fsmg_maml_tasks_config* c, const Episode& e, int32_t N, int32_t K, int32_t Q) {
    int rc = ensure_task_buffers(h, N);
    if (rc != FSMG_OK) return rc;
    ScopedTimer tm(h, "tasks");
    const size_t T = (size_t)h->T;
    h->task_loss_n = 0;
    for (int n = 0; n < N; ++n) {
        const int32_t* sup = e.sup + (size_t)n * K * T;
        const int32_t* qry = e.qry + (size_t)n * Q * T;
        const int32_t* slen = e.masked ? e.slen + (size_t)n * K : nullptr;
        const int32_t* qlen = e.masked ? e.qlen + (size_t)n * Q : nullptr;
        rc = maml_adapt_rows(h, sup, 1, K, c->inner_steps, c->inner_lr, e.on_device, slen, true);
        if (rc == FSMG_OK) rc = e.masked ? masked_query_pass(h, qry, qlen, 1, Q, e.on_device)
                                         : fsmg_forward_backward(h, qry, qry, 1, Q, 0, e.on_device);       // query rows at theta'_n
        if (rc == FSMG_OK && n == N - 1) rc = keep_theta_prime(h);
        if (rc == FSMG_OK) rc = fold_artist(h, n, N);
        if (rc != FSMG_OK) break;
    }
    if (rc != FSMG_OK) {                // theta comes back whatever happened; no fold is pending
        if (h->P_saved) {
            (void)keep_theta_prime(h);
            (void)restore_theta(h);
        }
        h->have_grads = false;
        h->msgd_pending = false;
        return rc;
    }
    // the buckets of an exchange are final behind the last fold, not behind the last pass
    HIPCK(h, hipEventRecord(h->ev_bucket[0], h->stream));
    HIPCK(h, hipEventRecord(h->ev_bucket[1], h->stream));
    h->bucket0_recorded = true;
    h->have_grads = true;
    h->msgd_pending = h->msgd_on;
    h->task_loss_n = N;
    return FSMG_OK;
}

int read_task_losses(fsmg_model* h, float* task_loss, int N) {
    HIPCK(h, hipMemcpyAsync(task_loss, h->d_task_loss, sizeof(float) * (size_t)N, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return FSMG_OK;
}

}  // namespace

// =========================================================================== C ABI
extern "C" {

int fsmg_maml_tasks_forward_backward(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                                     const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_tasks_args(h, c, support, query, support_len, query_len, N, K, Q);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    Episode e;
    if ((rc = locate_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    return tasks_forward_backward(h, c, e, N, K, Q);
}

int fsmg_maml_tasks_step(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                         const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* loss, float* task_loss) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_tasks_args(h, c, support, query, support_len, query_len, N, K, Q);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    Episode e;
    if ((rc = locate_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    auto fb = [&]() { return tasks_forward_backward(h, c, e, N, K, Q); };
    if (h->comm != nullptr) {           // per-rank adaptations (no communication), the folded gradient exchanged like a plain step's
        rc = dp_train_step_fn(h, loss, fb);
    } else {
        const uint64_t drop_p0 = h->drop_next;
        rc = fb();
        if (rc != FSMG_OK) return rc;
        rc = fsmg_apply_update(h, 1.0f, loss);
        if (is_retry(rc) && h->retry_armed) {        // same recovery as fsmg_maml_step: nothing was updated, repeat the whole call per step
            h->retry_armed = false;
            h->drop_next = drop_p0;
            rc = fb();
            if (rc == FSMG_OK) rc = fsmg_apply_update(h, 1.0f, loss);
        }
    }
    if (rc == FSMG_OK && task_loss != nullptr) rc = read_task_losses(h, task_loss, N);
    return rc;
}

int fsmg_maml_tasks_eval(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                         const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* nll, float* task_nll) {
    if (!h) return FSMG_ERR_INVALID;
    if (!nll) return fail(h, FSMG_ERR_INVALID, "null nll pointer");
    int rc = check_tasks_args(h, c, support, query, support_len, query_len, N, K, Q);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    Episode e;
    if ((rc = locate_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    const size_t T = (size_t)h->T;
    std::vector<float> per((size_t)N);
    double sum = 0.0;
    for (int n = 0; n < N; ++n) {       // artist n alone: fsmg_maml_eval's adaptation, query pass, restore and repeat for N = 1
        const int32_t* sup = e.sup + (size_t)n * K * T;
        const int32_t* qry = e.qry + (size_t)n * Q * T;
        rc = e.masked ? fsmg_maml_eval_masked(h, sup, qry, e.slen + (size_t)n * K, e.qlen + (size_t)n * Q, 1, K, Q, c->inner_steps, c->inner_lr,
                                              e.on_device, &per[(size_t)n])
                      : fsmg_maml_eval(h, sup, qry, 1, K, Q, c->inner_steps, c->inner_lr, e.on_device, &per[(size_t)n]);
        if (rc != FSMG_OK) return rc;
        sum += (double)per[(size_t)n];
    }
    *nll = (float)(sum / (double)N);
    if (task_nll) std::memcpy(task_nll, per.data(), sizeof(float) * (size_t)N);
    return FSMG_OK;
}

}  // extern "C"
