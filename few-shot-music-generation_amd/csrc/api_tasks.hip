// Per-artist MAML (include/fsmg.h "per-artist MAML"): the episode as a meta-batch of N tasks.  The train driver loops over
// the artists around maml_adapt and rows_pass (api_step.hip) on one-artist episodes and folds behind each; the eval driver is maml_eval
// per artist.
// Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the fold's kernel lives in tasks.hip.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace {

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
int tasks_episode(fsmg_model* h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query, const int32_t* support_len,
                  const int32_t* query_len, int32_t N, int32_t K, int32_t Q, Episode* e) {
    return locate_episode(h, c->table_id, c->use_table_lengths != 0, support, query, support_len, query_len, N, K, Q, c->tokens_on_device, e);
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

int tasks_forward_backward(fsmg_model* h, const fsmg_maml_tasks_config* c, const Episode& e) {
    const int N = e.N;
    int rc = lopt_check_train(h, c->inner_steps);
    if (rc == FSMG_OK) rc = ensure_task_buffers(h, N);
    if (rc != FSMG_OK) return rc;
    ScopedTimer tm(h, "tasks");
    h->task_loss_n = 0;
    for (int n = 0; n < N; ++n) {
        const Episode a = e.artist(n, h->T);
        rc = maml_adapt(h, a, c->inner_steps, c->inner_lr, true);
        if (rc == FSMG_OK) rc = rows_pass(h, a.qry, a.masked ? a.qlen : nullptr, 1, a.Q, a.on_device);       // query rows at theta'_n
        if (rc == FSMG_OK && h->lopt_on) rc = lopt_meta_gradient(h, n == 0, 1.0 / (double)N);    // G_n through the learned rule, GPhi's fold
        if (rc == FSMG_OK && n == N - 1) rc = keep_theta_prime(h);
        if (rc == FSMG_OK) rc = fold_artist(h, n, N);
        if (rc != FSMG_OK) break;
    }
    if (rc != FSMG_OK) {                // theta comes back whatever happened; no fold is pending
        (void)end_adaptation(h);
        h->msgd_pending = false;
        h->lopt_pending = false;
        return rc;
    }
    // the buckets of an exchange are final behind the last fold, not behind the last pass
    HIPCK(h, hipEventRecord(h->ev_bucket[0], h->stream));
    HIPCK(h, hipEventRecord(h->ev_bucket[1], h->stream));
    h->bucket0_recorded = true;
    h->have_grads = true;
    h->msgd_pending = h->msgd_on;
    h->lopt_pending = h->lopt_on;
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
    if ((rc = tasks_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    return tasks_forward_backward(h, c, e);
}

int fsmg_maml_tasks_step(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                         const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* loss, float* task_loss) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_tasks_args(h, c, support, query, support_len, query_len, N, K, Q);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    Episode e;
    if ((rc = tasks_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    // per-rank adaptations (no communication), the folded gradient exchanged or applied like fsmg_maml_step's; a repeat is the whole call's
    rc = step_with_update(h, loss, [&]() { return tasks_forward_backward(h, c, e); });
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
    if ((rc = tasks_episode(h, c, support, query, support_len, query_len, N, K, Q, &e)) != FSMG_OK) return rc;
    std::vector<float> per((size_t)N);
    double sum = 0.0;
    for (int n = 0; n < N; ++n) {       // artist n alone: maml_eval's prologue, adaptation, query pass, restore and repeat for N = 1
        rc = maml_eval(h, e.artist(n, h->T), c->inner_steps, c->inner_lr, &per[(size_t)n]);
        if (rc != FSMG_OK) return rc;
        sum += (double)per[(size_t)n];
    }
    *nll = (float)(sum / (double)N);
    if (task_nll) std::memcpy(task_nll, per.data(), sizeof(float) * (size_t)N);
    return FSMG_OK;
}

}  // extern "C"
