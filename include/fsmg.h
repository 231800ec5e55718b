/*
 * libfsmg -- C-ABI of the MI355X-native LSTM-baseline episodic train / eval step.
 *
 * This is the drop-in boundary for the hot path of AI-ON/Few-Shot-Music-Generation
 * (reference tree: /root/reference).  The reference has no FFI of its own: its only
 * device boundary is `self._sess.run(...)` inside the `models/` plugin
 * (src/models/lstm_baseline.py:104,125,150).  The entry points below are what a
 * Python `models.lstm_baseline.LSTMBaseline` plugin binds with ctypes instead of a
 * TensorFlow session; each one names the reference interface it replaces.
 *
 * Conventions
 *   - plain C, opaque handle, caller-allocated buffers, no C++ exceptions cross the boundary;
 *   - every function returns 0 on success or a negative FSMG_ERR_* code;
 *     fsmg_last_error(handle) (or fsmg_last_error(NULL) for create-time errors) has the text;
 *   - a handle is NOT thread-safe; all work of a handle is ordered on ONE HIP stream
 *     (its own, or the caller's when fsmg_config.stream is set);
 *   - "host" pointers are ordinary CPU memory, "device" pointers are HBM addresses on the
 *     handle's device (e.g. torch.Tensor.data_ptr()); token arrays are int32, C-contiguous,
 *     ids in [0, input_size) exactly as the reference's Episode.support / Episode.query
 *     (src/data/episode.py:63-74);
 *   - parameters cross the boundary in the REFERENCE's variable layout (tf names and
 *     shapes, src/models/lstm_baseline.py:39-40,44-49,60-62): embedding [V1,E],
 *     kernel_<l> [(in+H),4H] with gate column blocks i,j,f,o, bias_<l> [4H],
 *     softmax_w [H,V1], softmax_b [V1];  V1 = input_size + 1 (start word).
 *     Inside, they live padded and gate-interleaved (DESIGN.md "HBM layout").
 *   - there is no CPU fallback: without a gfx950 device fsmg_create fails with
 *     FSMG_ERR_NO_DEVICE.
 */
#ifndef FSMG_H
#define FSMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSMG_VERSION 600 /* 0.6.0 */
/* layout of struct fsmg_config AND of every other struct / flat-buffer layout a caller may hold (struct fsmg_stats, the padded
 * sizes fsmg_debug_dims reports): fsmg_create rejects any other value in .config_version, so a caller built against an older
 * header fails at create time instead of being overrun later.  4 (0.5.0): fsmg_stats grew (steps_skipped_peer_failure in 0.4.0,
 * xov_selfcheck_mismatches now); hidden sizes that no persistent kernel takes at a multiple of 16 pad to a multiple of 64
 * (200 -> 256, not 208: every padded offset behind fsmg_debug_read / fsmg_debug_dims moved in 0.4.0 without a version bump). */
#define FSMG_CONFIG_VERSION 4

enum {
    FSMG_OK = 0,
    FSMG_ERR_INVALID = -1,     /* bad argument / config value                        */
    FSMG_ERR_NO_DEVICE = -2,   /* no usable HIP device (no CPU fallback exists)      */
    FSMG_ERR_HIP = -3,         /* a HIP runtime call failed                          */
    FSMG_ERR_NOMEM = -4,       /* host or device allocation failed                   */
    FSMG_ERR_NAME = -5,        /* unknown parameter / buffer name                    */
    FSMG_ERR_SIZE = -6,        /* element count does not match the named tensor      */
    FSMG_ERR_TOKEN_RANGE = -7, /* a token id was outside [0, input_size)             */
    FSMG_ERR_STATE = -8,       /* call sequence error (e.g. apply without backward)  */
    /* the step was SKIPPED on the device (parameters, Adam state and global_step untouched) and the handle has changed how it runs
     * the next one: repeat the call.  fsmg_train_step / _indexed / fsmg_maml_* repeat it themselves when a loss is read back. */
    FSMG_ERR_TIMEOUT = -9,         /* a persistent kernel's hand-off or gate timed out (its blocks were not co-resident, or two launches that must
                                      run side by side did not): the handle runs one launch per time step for `fallback_steps` steps */
    FSMG_ERR_SOFTMAX_RANGE = -10   /* a row's sum of exp(logit) or its target's exp(logit) left the fp32 range of the shift-free fused softmax:
                                      the handle takes the cross-entropy pass with the shifted softmax from here on (nothing else changes) */
};

enum { FSMG_CLIP_TF1_SLICES = 0, FSMG_CLIP_DENSE = 1 };
/* arithmetic of the dense contractions: AUTO = BX3 (every operand split exactly into three bf16 pieces, the six partial products
 * >= 2^-23 of the fp32 product summed on the bf16 matrix pipe: each product to within half an fp32 ulp, fp32 accumulation:
 * DESIGN.md section 4); F32 = v_mfma_f32_32x32x2_f32 */
enum { FSMG_GEMM_AUTO = 0, FSMG_GEMM_BX3 = 1, FSMG_GEMM_F32 = 2 };
/* order of a pass: AUTO picks from the shapes; SINGLE_STREAM = one stream, serial; TWO_STREAM = projection GEMMs on an
 * auxiliary stream beside the recurrence (eager); XCD_PARTITIONED = the bf16-split recurrence packed on ceil(rows / 16) XCDs, the
 * projection / its weight gradient as work-queue GEMMs on the other XCDs beside it (hidden 512, one layer; AUTO picks it there) */
enum { FSMG_SCHEDULE_AUTO = 0, FSMG_SCHEDULE_SINGLE_STREAM = 1, FSMG_SCHEDULE_TWO_STREAM = 2, FSMG_SCHEDULE_XCD_PARTITIONED = 3 };
/* recurrent kernels: AUTO = the fastest family the shape admits; PER_STEP = one launch per time step; COLUMN_SPLIT = persistent,
 * gate columns over the chip (round 1); XCD_LOCAL = persistent, rows over the XCDs (hidden size 512) */
enum { FSMG_RECURRENCE_AUTO = 0, FSMG_RECURRENCE_PER_STEP = 1, FSMG_RECURRENCE_COLUMN_SPLIT = 2, FSMG_RECURRENCE_XCD_LOCAL = 3 };

typedef struct fsmg_model* fsmg_handle;

/* Model / optimiser configuration == the YAML keys the reference plugin reads
 * (src/models/lstm_baseline.py:21-29,80; src/models/tf_model.py:81). */
typedef struct fsmg_config {
    int32_t input_size;      /* config['input_size']: vocabulary WITHOUT the start word        */
    int32_t max_len;         /* config['max_len'] = T                                         */
    int32_t embedding_size;  /* config['embedding_size'] = E                                  */
    int32_t hidden_size;     /* config['hidden_size'] = H                                     */
    int32_t n_layers;        /* config['n_layers'] = L                                        */
    float lr;                /* config['lr']                                                  */
    float max_grad_norm;     /* config['max_grad_norm']                                       */
    float n_decay;           /* config['n_decay'] (lr halves every n_decay steps, continuous) */
    int32_t clip_norm_mode;  /* FSMG_CLIP_TF1_SLICES (reference behaviour) or FSMG_CLIP_DENSE */
    int32_t device;          /* HIP device ordinal                                            */
    int32_t max_sequences;   /* sequences per training episode (N*(K+Q)): initial activation capacity (grows on demand)
                                and the row count the recurrent kernel family is chosen for (hidden 512, > 64 rows: the
                                bf16-split XCD-local kernels); 0 = 45 */
    int32_t use_graph;       /* 1: replay the per-timestep launch chains as hipGraphs         */
    void* stream;            /* optional caller hipStream_t; NULL = the library creates one   */
    void* state_arena;       /* optional caller-owned DEVICE memory for params+grads+Adam state
                                (fsmg_state_bytes() bytes, 256-B aligned); NULL = hipMalloc  */
    uint64_t state_arena_bytes;
    /* ---- since config version 3: what used to be environment variables read at create time.  The variables still exist as
     * debugging overrides (FSMG_GEMM, FSMG_OVERLAP, FSMG_XCD_OVERLAP, FSMG_PERSISTENT, FSMG_XCD, FSMG_DP_SPLIT, ...: they win) */
    int32_t config_version;     /* must be FSMG_CONFIG_VERSION: a caller built against another header is refused            */
    int32_t gemm;               /* FSMG_GEMM_*                                                                               */
    int32_t schedule;           /* FSMG_SCHEDULE_*                                                                           */
    int32_t recurrence;         /* FSMG_RECURRENCE_*                                                                         */
    int32_t dp_split_backward;  /* 1: fsmg_forward_backward replays two graphs and bucket 0 of the gradient exchange
                                   (softmax gradients) is final behind the first one (fsmg_stream_wait_bucket), which ends
                                   behind the projection gradients; 2: the first graph ends behind the last recurrent
                                   chain instead (a collective started before a chain that needs every CU only delays it)   */
    int32_t reserved[7];        /* zero                                                                                       */
} fsmg_config;

/* ---- lifetime -------------------------------------------------------------------------- */
int fsmg_version(void);
const char* fsmg_last_error(fsmg_handle h);
/* bytes a caller-provided state arena must have for this config */
uint64_t fsmg_state_bytes(const fsmg_config* cfg);
/* replaces TFModel.__init__ (session + graph build, src/models/tf_model.py:80-97) */
int fsmg_create(const fsmg_config* cfg, fsmg_handle* out);
int fsmg_destroy(fsmg_handle h);
int fsmg_synchronize(fsmg_handle h);

/* ---- parameters, optimiser state, checkpoints ------------------------------------------ */
/* replaces the variable initialisation of recover_or_init (src/models/tf_model.py:16-25,127-129):
 * Glorot-uniform for every matrix AND softmax_b, zeros for LSTM biases;
 * also zeroes Adam m/v and global_step. */
int fsmg_init_params(fsmg_handle h, uint64_t seed);
int fsmg_num_params(fsmg_handle h);
/* name (tf variable name without scope), rows, cols (cols = 1 for vectors) of parameter idx */
int fsmg_param_info(fsmg_handle h, int idx, char* name, int name_cap, int64_t* rows, int64_t* cols);
/* replace Saver.restore / Saver.save of a variable (src/models/tf_model.py:96-114); host
 * float32 buffers in the reference layout, count = rows*cols */
int fsmg_set_param(fsmg_handle h, const char* name, const float* host, int64_t count);
int fsmg_get_param(fsmg_handle h, const char* name, float* host, int64_t count);
/* Adam slots of a variable (what a TF checkpoint holds besides weights) */
int fsmg_set_opt_state(fsmg_handle h, const char* name, const float* m, const float* v, int64_t count);
int fsmg_get_opt_state(fsmg_handle h, const char* name, float* m, float* v, int64_t count);
int fsmg_set_step(fsmg_handle h, int64_t global_step);
int fsmg_get_step(fsmg_handle h, int64_t* global_step);
/* gradient of the last backward, reference layout, before clipping (parity tests) */
int fsmg_get_grad(fsmg_handle h, const char* name, float* host, int64_t count);

/* ---- the hot path ---------------------------------------------------------------------- */
/* replaces LSTMBaseline.train (src/models/lstm_baseline.py:89-113): support [N,K,T] and
 * query [N,Q,T] are flattened support-rows-first, shifted against the start word on the
 * device, forward + BPTT + clip_by_global_norm + Adam + global_step++.  *loss receives the
 * mean NLL computed with the PRE-update parameters; passing loss == NULL skips the
 * device->host readback (the loss stays in the handle's ring, see fsmg_read_losses).
 * tokens_on_device != 0: support/query are device pointers (episode pool resident in HBM). */
int fsmg_train_step(fsmg_handle h, const int32_t* support, const int32_t* query,
                    int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device, float* loss);

/* Episode-parallel form of the same step: forward + backward only; the flat fp32
 * gradient buffer (fsmg_grad_buffer) is then summed across ranks by the host (one RCCL
 * all-reduce), and fsmg_apply_update(grad_scale = 1/world) clips and applies Adam identically
 * on every rank. */
int fsmg_forward_backward(fsmg_handle h, const int32_t* support, const int32_t* query,
                          int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device);
/* device address + element count of the flat gradient buffer; the last FSMG_GRAD_TAIL floats
 * are scalars that must be reduced with it: [0] = sum of squared embedding-slice gradients,
 * [1] = loss, [2] = non-zero when a persistent recurrent kernel of this rank timed out (its gradients are garbage):
 * fsmg_apply_update then leaves parameters, Adam state and step counter alone on every rank and, when it reads the
 * loss back, returns FSMG_ERR_TIMEOUT after switching the handle to one launch per time step -- repeat the step;
 * [3] = non-zero when this rank's batch held a token id outside [0, input_size): summed like [2], so EVERY rank skips the
 * update (replicas stay identical) and every rank's read-back returns FSMG_ERR_TOKEN_RANGE;
 * [4] = non-zero when this rank's pass failed on the host before the exchange (library-owned exchange: the rank still joins
 * the collectives so that no peer blocks): every rank skips the update, peers' read-backs return FSMG_ERR_STATE;
 * [5] = non-zero when a row of this rank's logits left the range of the shift-free fused softmax: summed like [2], every rank skips
 * the update, switches to the cross-entropy pass with the shifted softmax and returns FSMG_ERR_SOFTMAX_RANGE -- repeat the step */
#define FSMG_GRAD_TAIL 16
int fsmg_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count);
int fsmg_apply_update(fsmg_handle h, float grad_scale, float* loss);
/* Bucketed form of the gradient exchange, so that communication overlaps the rest of the backward pass:
 *   bucket 0 = softmax_w + softmax_b gradients (final as soon as the dW GEMM retires, 56 % of the bytes at cfg-B)
 *   bucket 1 = every other gradient, bucket 2 = the FSMG_GRAD_TAIL scalars (both final when backward ends).
 * fsmg_grad_bucket returns the device range of a bucket; fsmg_stream_wait_bucket makes `stream` (the caller's
 * communication hipStream_t) wait until that bucket of the LAST fsmg_forward_backward is final. */
#define FSMG_NUM_BUCKETS 3
int fsmg_grad_bucket(fsmg_handle h, int32_t bucket, void** device_ptr, int64_t* count);
int fsmg_stream_wait_bucket(fsmg_handle h, void* stream, int32_t bucket);

/* The gradient exchange INSIDE the library ("fsmg_allreduce_grads internal to train_step when world > 1").
 * With a communicator attached, fsmg_train_step / fsmg_train_step_indexed / fsmg_maml_step are the episode-parallel step by
 * themselves: forward + backward graph(s) -> ncclAllReduce(SUM) of the three gradient buckets on the library's own
 * communication stream (bucket 0 as soon as the projection gradients are final when fsmg_config.dp_split_backward is set) ->
 * clip + Adam with grad_scale = 1 / world_size; the caller (PyTorch or anything else) only owns the memory.  RCCL is looked up
 * at run time (dlopen of the librccl.so already in the process, else /opt/rocm/lib): no link-time dependency.
 *   fsmg_comm_unique_id        rank 0: a fresh ncclUniqueId to hand to the other ranks by whatever means the job has;
 *   fsmg_comm_init             every rank: ncclCommInitRank on the handle's device (a collective call);
 *   fsmg_comm_attach           instead of the two above: an ncclComm_t the caller already owns (never destroyed by the library);
 *   fsmg_comm_broadcast_state  parameters, Adam slots and global_step of rank `root` to every rank (after init / restore);
 *   fsmg_comm_release          detach (and destroy a communicator the library created).
 * fsmg_forward_backward / fsmg_apply_update stay for callers that own the exchange. */
#define FSMG_COMM_ID_BYTES 128
int fsmg_comm_unique_id(char id[FSMG_COMM_ID_BYTES]);
int fsmg_comm_init(fsmg_handle h, const char id[FSMG_COMM_ID_BYTES], int32_t world_size, int32_t rank);
int fsmg_comm_attach(fsmg_handle h, void* nccl_comm, int32_t world_size, int32_t rank);
int fsmg_comm_broadcast_state(fsmg_handle h, int32_t root);
int fsmg_comm_release(fsmg_handle h);

/* Device-resident episode table.  The reference fills an episode from a host cache of per-song rows
 * (src/data/episode.py:62-74, src/data/dataset.py:187-199); here the packed split -- int32 [n_songs][max_len], the
 * `.npy` sidecars of the split in artist/song order -- is uploaded once and an episode is N*K + N*Q ROW INDICES gathered on
 * the GPU.  table_id in [0, 4) (e.g. 0 train, 1 val, 2 test).  An index outside [0, n_songs) -> FSMG_ERR_TOKEN_RANGE. */
int fsmg_upload_table(fsmg_handle h, int32_t table_id, const int32_t* host_table, int64_t n_songs);
int fsmg_forward_backward_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                  int32_t N, int32_t K, int32_t Q);
int fsmg_train_step_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                            int32_t N, int32_t K, int32_t Q, float* loss);

/* replaces LSTMBaseline.eval (src/models/lstm_baseline.py:115-133): query-only mean NLL,
 * no state change. */
int fsmg_eval_step(fsmg_handle h, const int32_t* query, int32_t N, int32_t Q,
                   int32_t tokens_on_device, float* nll);
/* n_episodes independent eval calls in one pass: queries [n_episodes,N,Q,T] -> nll[n_episodes]
 * (what train.evaluate's loop over model.eval computes, src/train/train.py:27-33) */
int fsmg_eval_batch(fsmg_handle h, const int32_t* queries, int32_t n_episodes, int32_t N, int32_t Q,
                    int32_t tokens_on_device, float* nll);

/* ---- per-song lengths: the padding-masked loss ------------------------------------------------
 * The same passes for songs shorter than max_len = T.  Every row b of a pass has a length len[b] in [1, T]; position t of row b
 * is scored iff t < len[b] (its inputs are [start, x_0 .. x_{t-1}], its target x_t), and with n_valid = the sum of the lengths
 *   loss = sum_{b, t < len[b]} ce[b][t] / (n_valid + 1e-12),   dlogits[b][t] = (softmax - onehot) * w[b][t],
 *   w[b][t] = t < len[b] ? (float)(1 / ((double)n_valid + 1e-12)) : 0
 * -- TF's sequence_loss with 0 / 1 weights, averaged across time steps and batch.  All T steps of every row are still computed.
 * Two laws: with every length T a masked call has the unmasked call's bits (loss, gradients, tail, updated state); and the
 * tokens at t >= len[b] never matter (a position behind a song's end gets fixed ids on the device, and its row enters every
 * gradient with an exact 0) -- they must still be in range.  The range check of the fused softmax covers all rows.
 * support_len [N*K] and query_len [N*Q] follow the token pointers and live where they do: tokens_on_device covers both.  Host
 * lengths are checked before any device work (one outside [1, T], or a NULL pointer: FSMG_ERR_INVALID, nothing touched); device
 * lengths are checked by the kernel that builds the weights, which raises the flag of an out-of-range token: the step is
 * skipped on the device, the read-back returns FSMG_ERR_TOKEN_RANGE, and in an episode-parallel job every rank skips.
 * Everything else is the unmasked call's: the loss ring, fsmg_apply_update behind fsmg_forward_backward_masked (loss in
 * tail[1]), buckets, time-out and range retries, the library-owned exchange.  In an episode-parallel job each rank normalises
 * by its OWN n_valid and grad_scale = 1 / world takes the mean of those: the unmasked convention, a mean of per-episode means
 * (not a mean over all ranks' tokens).  A handle may alternate masked and unmasked calls freely.
 * fsmg_eval_batch_masked: query_len [n_episodes*N*Q], each episode's NLL over its own n_valid.
 * fsmg_upload_table_lengths: the lengths [n_songs] of the token table uploaded under table_id (FSMG_ERR_STATE without a table
 * of the same n_songs; every length checked here; uploading the table again drops them); the indexed masked calls gather a
 * row's length with the row (the host sends indices only) and return FSMG_ERR_STATE for a table without lengths.
 * fsmg_debug_read: "row_weight" = the T*B weights of the last masked pass in device row order t*B + b, "n_valid" = its groups'. */
int fsmg_train_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                           const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device, float* loss);
int fsmg_forward_backward_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                                 const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t tokens_on_device);
int fsmg_eval_step_masked(fsmg_handle h, const int32_t* query, const int32_t* query_len, int32_t N, int32_t Q,
                          int32_t tokens_on_device, float* nll);
int fsmg_eval_batch_masked(fsmg_handle h, const int32_t* queries, const int32_t* query_len, int32_t n_episodes, int32_t N,
                           int32_t Q, int32_t tokens_on_device, float* nll);
int fsmg_upload_table_lengths(fsmg_handle h, int32_t table_id, const int32_t* lengths, int64_t n_songs);
int fsmg_train_step_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                   int32_t N, int32_t K, int32_t Q, float* loss);
int fsmg_forward_backward_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                         int32_t N, int32_t K, int32_t Q);

/* ---- cfg-E (BASELINE.json configs[4]): MAML-style inner / outer loop, first order.
 * The reference has no code for it (READING_LIST.md:5-7 names the direction); semantics: DESIGN.md "cfg-E", oracle:
 * oracle/lstm_oracle.py maml_step / maml_eval.  theta' starts at theta and takes `inner_steps` steps
 *   theta' <- theta' - inner_lr * clip_by_global_norm(grad of the SUPPORT rows' mean NLL at theta', max_grad_norm);
 * the outer gradient is the gradient of the QUERY rows' mean NLL with respect to theta' (no derivative through the inner
 * steps); theta is restored before anything is updated.
 *   fsmg_maml_forward_backward  leaves that gradient (+ the query loss in the tail) in the flat gradient buffer, theta and
 *                               Adam state untouched: all-reduce it across ranks, then fsmg_apply_update(1/world);
 *   fsmg_maml_step              = the two on one GPU (clip + Adam on theta, global_step++); *loss = query NLL at theta';
 *   fsmg_maml_eval              few-shot evaluation: adapt on the support set, query NLL at theta', no state change. */
int fsmg_maml_forward_backward(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K,
                               int32_t Q, int32_t inner_steps, float inner_lr, int32_t tokens_on_device);
int fsmg_maml_step(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                   int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* loss);
int fsmg_maml_eval(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q,
                   int32_t inner_steps, float inner_lr, int32_t tokens_on_device, float* nll);
/* the same two on the device-resident split table (fsmg_upload_table): the episode is N*K + N*Q ROW INDICES (host int32) */
int fsmg_maml_forward_backward_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                       int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr);
int fsmg_maml_step_indexed(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                           int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, float* loss);

/* ---- cfg-E with per-song lengths: the padding-masked loss of DESIGN.md 20 in every pass of the MAML-style step.
 * support_len [N*K] and query_len [N*Q], every one in [1, T]; position t of row b is scored iff t < len[b].  Inner step i:
 *   theta'_{i+1} = theta'_i - inner_lr * clip_by_global_norm(grad of L_sup(theta'_i), max_grad_norm),
 *   L_sup = sum over support (b, t < len[b]) of ce / (n_valid_sup + 1e-12),  n_valid_sup = the sum of the support lengths
 * (one group of N*K rows; both clip-norm modes as in the unmasked call).  The outer gradient is the gradient of L_qry, the same sum
 * over the query rows / (n_valid_qry + 1e-12), with respect to theta', first order; the loss / NLL returned is L_qry(theta'); theta
 * is restored whatever happens.  Two laws, as in DESIGN.md 20: with every length T a call has its unmasked twin's bits (loss,
 * gradients, tail, theta', updated state, NLL); and the tokens at t >= len[b] never matter (fixed ids stand in for them on the
 * device) -- they must still be in range.
 * The lengths live where the tokens do (tokens_on_device covers all four pointers).  Host lengths are checked before any device
 * work: one outside [1, T] or a NULL pointer gives FSMG_ERR_INVALID with nothing touched -- theta, the saved copy of theta, the
 * gradient buffer.  Device lengths are checked by the kernel that builds each pass's weights, which raises the token-range flag:
 * every update of the call is skipped on the device and the call returns FSMG_ERR_TOKEN_RANGE.
 * Everything the unmasked twins promise holds: theta, Adam slots, global_step and the loss ring are untouched by
 * _forward_backward_masked / _eval_masked; the gradient buffer and the recurrent-launch counters are used as they use them;
 * fsmg_apply_update follows _forward_backward_masked; a time-out repeats the whole call -- adaptation, lengths and all -- on
 * per-step launches; fsmg_debug_set("keep_adapted") / "adapted:<name>" work.  With a communicator attached fsmg_maml_step_masked is
 * the episode-parallel step: each rank normalises by its OWN n_valid_qry and grad_scale = 1 / world takes the mean.
 * Each of the inner_steps + 1 train passes costs the two launches and the one length copy a masked train pass adds (the row
 * weights, the masked loss sum), the query pass of _eval_masked one launch (the row weights).
 * The _indexed_masked forms gather each row's length with the row (fsmg_upload_table_lengths; a table without lengths:
 * FSMG_ERR_STATE, nothing touched). */
int fsmg_maml_forward_backward_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                                      const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t inner_steps,
                                      float inner_lr, int32_t tokens_on_device);
int fsmg_maml_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                          const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr,
                          int32_t tokens_on_device, float* loss);
int fsmg_maml_eval_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                          const int32_t* query_len, int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr,
                          int32_t tokens_on_device, float* nll);
int fsmg_maml_forward_backward_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx,
                                              const int32_t* query_idx, int32_t N, int32_t K, int32_t Q, int32_t inner_steps,
                                              float inner_lr);
int fsmg_maml_step_indexed_masked(fsmg_handle h, int32_t table_id, const int32_t* support_idx, const int32_t* query_idx,
                                  int32_t N, int32_t K, int32_t Q, int32_t inner_steps, float inner_lr, float* loss);

/* replaces LSTMBaseline.sample (src/models/lstm_baseline.py:135-156): greedy argmax decode of
 * `num` tokens from the start word and a zero state (the support set is ignored there; a carried state: fsmg_dstate_*). */
int fsmg_sample(fsmg_handle h, int32_t num, int32_t* out_tokens);

/* ---- batched on-device generation (DESIGN.md "Batched generation").  n_seq independent rows, each the input sequence
 * [start, primer[b][0..P-1], g_0, g_1, ...] (start = input_size, the training shift), zero initial state; token g_t is drawn from
 * the output after the input just before it (P = 0: the first token comes from the start word's output, like fsmg_sample).
 * logit = h_L . softmax_w + softmax_b over all V1 = input_size + 1 columns.  The draw is Gumbel-max: g_t = argmax over the allowed
 * set of logit_v / temperature + gumbel_v, lowest index on ties, gumbel_v = -log(-log(u)), u = ((x >> 8) + 0.5) * 2^-24, x = word
 * v & 3 of Philox4x32-10(key = (seed & 0xffffffff, seed >> 32), counter = (v >> 2, t, b, 0)) -- b the row index in the call.
 * Allowed set: every column when top_k is 0 or V1, else the columns whose logit is >= the top_k-th largest (ties included).
 * temperature == 0 (or top_k == 1): the argmax of the logits, no noise.  out_logprob[b][t] = logit_tok - logsumexp(all V1 logits):
 * the untempered, untruncated model log-probability.  A row's tokens and log-probs are bitwise independent of n_seq and of the
 * other rows.  fsmg_generate changes no handle state (parameters, Adam moments, global_step, the loss ring, gradients, statistics,
 * captured graphs).  fsmg_maml_generate first adapts like fsmg_maml_eval and restores theta whatever happens; exactly as fsmg_maml_eval, its inner
 * forward / backward passes overwrite the gradient buffer and advance the recurrent-launch counters of fsmg_stats (xcd_launches,
 * persistent_launches, step_launches), and a time-out inside them is counted and handled like any other (timeouts, fallback_steps_left).
 * Parameters, Adam moments, global_step and the loss ring stay as they were.
 * Errors: FSMG_ERR_INVALID for a bad config (version, n_seq < 1, num < 0, primer_len < 0, temperature negative or not finite, top_k
 * outside [0, V1], nonzero reserved fields); FSMG_ERR_TOKEN_RANGE for a primer id outside [0, input_size) (out_tokens left
 * unwritten).  A row whose logits are not comparable (NaN) still yields a token in [0, V1). */
#define FSMG_GEN_CONFIG_VERSION 1
typedef struct fsmg_gen_config {
    int32_t version;          /* FSMG_GEN_CONFIG_VERSION, else FSMG_ERR_INVALID            */
    int32_t n_seq;            /* B >= 1 independent sequences                              */
    int32_t num;              /* tokens generated per sequence, >= 0                       */
    int32_t primer_len;       /* P >= 0 primer tokens per sequence (teacher-forced)        */
    float temperature;        /* >= 0, finite; 0 = greedy argmax (no noise)                */
    int32_t top_k;            /* 0 = all V1 columns, else 1..V1                            */
    uint64_t seed;
    int32_t primer_on_device; /* primer pointer is host (0) or device (1)                  */
    int32_t reserved[7];      /* must be 0                                                 */
} fsmg_gen_config;

/* primer [B,P] (NULL if P == 0), out_tokens host [B,num], out_logprob host [B,num] or NULL */
int fsmg_generate(fsmg_handle h, const fsmg_gen_config* g, const int32_t* primer, int32_t* out_tokens, float* out_logprob);
/* adapt on support [n_support_rows, max_len] (host, or device when support_on_device) for inner_steps clipped SGD steps of
 * inner_lr, generate at theta', restore theta */
int fsmg_maml_generate(fsmg_handle h, const fsmg_gen_config* g, const int32_t* support, int32_t n_support_rows, int32_t inner_steps,
                       float inner_lr, int32_t support_on_device, const int32_t* primer, int32_t* out_tokens, float* out_logprob);

/* ---- sampling filters for fsmg_generate (DESIGN.md "Sampling filters"): nucleus (top-p), min-p and a repetition penalty.
 * At generated position t of row b, let z be the V1 logits exactly as fsmg_generate computes them and T its temperature.
 * 1. Penalty (theta = repetition_penalty).  The context is primer[b][0..P-1], g_0 .. g_{t-1}; the start word is not part of it.
 *    With repeat_window n > 0 take the last min(n, P + t) context tokens, with n = 0 all of them; S = the distinct ids there.
 *    z'_v = z_v > 0 ? fl(z_v / theta) : fl(z_v * theta) for v in S (once per id, however often it occurs), z'_v = z_v otherwise.
 *    NaN stays NaN.
 * 2. Top-k (fsmg_gen_config.top_k, fsmg_generate's rule, on z'): A = the columns with z' >= the top_k-th largest z', ties included
 *    (NaN columns are never in A; with fewer than top_k comparable columns, every comparable column).
 * 3. Min-p (min_p = m > 0): keep the v in A with (z'_v - z'_max) / T >= ln m, z'_max the maximum z' over A.
 * 4. Top-p (0 < top_p = p < 1): for q = softmax(z' / T) renormalised over the survivors of 3, keep v iff the mass of the
 *    survivors with strictly larger z' is < p.  The top column always stays, and so does every tie at the boundary.
 * 5. Draw: fsmg_generate's Gumbel-max over the final set, same Philox counter (v >> 2, t, b, 0), same tie rule (lowest index).
 *    T = 0 or top_k = 1: the argmax of z' (lowest index).  NaN columns are never drawn while any comparable column exists; a row
 *    without a comparable logit still yields a column in [0, V1).
 * 6. out_logprob is unchanged: z_tok - logsumexp(all raw z), the untempered, unfiltered model log-probability, with the lse
 *    bitwise the number fsmg_generate uses.
 * Neutral filters (f == NULL, or top_p in {0, 1}, min_p = 0 and repetition_penalty in {0, 1}) give fsmg_generate's tokens and
 * log-probs bitwise.  The rest of fsmg_generate's contract holds with filters on: bitwise deterministic, a row's output bitwise
 * independent of n_seq and of the other rows, no handle state changed (the MAML variant: fsmg_maml_generate's documented side
 * effects only).  Top-p sums the masses in fixed point (2^-32 of the top column's weight), exactly and in a fixed order; its
 * boundary may differ from exact arithmetic only for a column whose mass-ahead is within about V1 * 2^-32 of p.
 * Errors: FSMG_ERR_INVALID for everything fsmg_generate refuses, a wrong filters version or nonzero reserved fields, top_p or
 * min_p outside [0, 1] or NaN, repetition_penalty negative or not finite, repeat_window < 0, and a penalty at V1 > 2^20;
 * FSMG_ERR_TOKEN_RANGE for a primer id outside [0, input_size). */
#define FSMG_GEN_FILTERS_VERSION 1
typedef struct fsmg_gen_filters {
    int32_t version;            /* FSMG_GEN_FILTERS_VERSION                                       */
    float   top_p;              /* 0 or 1 = off, else (0, 1)                                      */
    float   min_p;              /* 0 = off, else (0, 1]                                           */
    float   repetition_penalty; /* 0 or 1 = off, else finite > 0                                 */
    int32_t repeat_window;      /* >= 0; 0 = the whole context                                    */
    int32_t reserved[8];        /* must be 0                                                      */
} fsmg_gen_filters;

/* fsmg_generate with filters f (NULL: none) */
int fsmg_generate_filtered(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f,
                           const int32_t* primer, int32_t* out_tokens, float* out_logprob);
/* fsmg_maml_generate with filters f (NULL: none) */
int fsmg_maml_generate_filtered(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f,
                                const int32_t* support, int32_t n_support_rows, int32_t inner_steps, float inner_lr,
                                int32_t support_on_device, const int32_t* primer, int32_t* out_tokens, float* out_logprob);
/* fsmg_maml_generate_filtered with per-song support lengths: support_len [n_support_rows], every one in [1, max_len],
 * where the support tokens are (support_on_device covers both); every inner step is fsmg_maml_eval_masked's, over the positions
 * t < support_len[b] only, and the generation at theta' is fsmg_maml_generate_filtered's, launch for launch.  A NULL support_len or a
 * host length out of range: FSMG_ERR_INVALID before any device work; a device length out of range raises the token-range flag in
 * the kernel that builds the weights: FSMG_ERR_TOKEN_RANGE, outputs unwritten.  Side effects and the time-out repeat: the twin's. */
int fsmg_maml_generate_filtered_masked(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f,
                                       const int32_t* support, const int32_t* support_len, int32_t n_support_rows,
                                       int32_t inner_steps, float inner_lr, int32_t support_on_device, const int32_t* primer,
                                       int32_t* out_tokens, float* out_logprob);

/* ---- constrained decoding: restrict what fsmg_generate_filtered may draw, on the device, inside the pick.
 * A constraint is one immutable device object per vocabulary, made of three independent mechanisms, each of which may be absent:
 *   bias         bias[V1] is added to the logit; -inf bans a column (+inf and NaN are refused).  NULL: zeros.
 *   automaton    token_class[V1] in [0, C), next_state[S][C] in [-1, S) (-1 forbids every token of that class in that state),
 *                start_state in [0, S); 1 <= S <= 256, 1 <= C <= 64.  Absent (both tables NULL, n_states = n_classes = 0):
 *                S = C = 1 with everything allowed.
 *   slots        slot_open[V1] and slot_close[V1] in [-1, K), 0 <= K <= 4096, a token with at most one role.  A token that opens
 *                slot k is allowed only while k is closed and drawing it opens k; one that closes k only while k is open, and
 *                drawing it closes k.  NULL arrays: no token has that role.
 * A row's constraint state is (state, open[ceil(K / 32)], dead_ends); bit k of open is bit k & 31 of word k >> 5.
 * At generated position t of row b let z be the logits row exactly as fsmg_generate computes it and (s, open) the row's state.
 *   Omega = { v : bias_v > -inf, next_state[s][token_class[v]] >= 0, v's slot rule holds }
 *   z^c_v = fl(z_v + bias_v) for v in Omega, -inf otherwise.
 * Steps 1 to 5 of fsmg_generate_filtered run on z^c in place of z, unchanged: same Philox counter (v >> 2, t, b, 0), seed and tie
 * rule.  A column outside Omega is never drawn while Omega is non-empty, at temperature 0 too; when every allowed column's z^c is
 * -inf or NaN the pick is the lowest column of Omega.  Dead end (Omega empty): the position is picked as if no constraint were
 * given (z^c = z over all columns), the constraint state stays as it is and the row's dead_ends goes up by one -- nothing hangs,
 * nothing is refused, the caller reads the counter.  out_logprob is unchanged: z_tok - logsumexp(all raw z), the lse bitwise
 * fsmg_generate's.  After the pick s <- next_state[s][token_class[tok]] and tok's slot is flipped.  Primer tokens advance the
 * state in order before the first pick (the start word is no primer token and advances nothing); a primer token that is not
 * allowed where it stands: a host primer gives FSMG_ERR_INVALID before any device work, a device primer raises the primer flag,
 * FSMG_ERR_TOKEN_RANGE with the outputs unwritten.
 * cstate_io (may be NULL, as may each of its arrays) carries the rows' states: read at the start of the call (NULL: start_state,
 * every slot closed, zero dead ends), written at its end.  state [B], open [B][ceil(K / 32)], dead_ends [B].
 * con == NULL: every call is bitwise its unconstrained twin and launches that twin's kernels (cstate_io is not touched).
 * The rest of fsmg_generate_filtered's contract holds: bitwise deterministic, a row's output independent of n_seq and of the
 * other rows, no handle state changed.  A constraint outlives the calls that use it and is freed by fsmg_constraint_destroy or with
 * the handle.  Beam search under a constraint: fsmg_beam_search_constrained, below.  Not covered: the cache-conditioned generators
 * and fsmg_dyneval_generate.
 * Errors: fsmg_constraint_create returns FSMG_ERR_INVALID for a bad version or nonzero reserved words, n_columns that is not the
 * handle's V1 = input_size + 1, V1 > 2^19, S, C or K outside their limits, one automaton table without the other, any index out of range, a
 * token with both slot roles, a bias of +inf or NaN.  The generate calls: what their unconstrained twins refuse; FSMG_ERR_INVALID
 * for a constraint this handle does not own, a cstate_io state outside [0, S), negative dead_ends or an open bit at or above K. */
#define FSMG_CONSTRAINT_CONFIG_VERSION 1
typedef struct fsmg_constraint_s* fsmg_constraint;
struct fsmg_dstate_s;           /* a decode state (fsmg_dstate, below) */
typedef struct fsmg_constraint_config {
    int32_t version;            /* FSMG_CONSTRAINT_CONFIG_VERSION                                 */
    int32_t n_columns;          /* V1 = input_size + 1 of the handle                              */
    int32_t n_states;           /* S in [1, 256]; 0 with NULL tables: no automaton                */
    int32_t n_classes;          /* C in [1, 64];  0 with NULL tables: no automaton                */
    int32_t n_slots;            /* K in [0, 4096]                                                 */
    int32_t start_state;        /* in [0, S)                                                      */
    int32_t reserved[10];       /* must be 0                                                      */
    const float*   bias;        /* host [V1] or NULL                                              */
    const int32_t* token_class; /* host [V1] or NULL                                              */
    const int32_t* next_state;  /* host [S][C] or NULL                                            */
    const int32_t* slot_open;   /* host [V1] or NULL                                              */
    const int32_t* slot_close;  /* host [V1] or NULL                                              */
} fsmg_constraint_config;
typedef struct fsmg_constraint_state {
    int32_t*  state;            /* host [B] or NULL                                               */
    uint32_t* open;             /* host [B][ceil(K / 32)] or NULL                                 */
    int32_t*  dead_ends;        /* host [B] or NULL                                               */
} fsmg_constraint_state;

int fsmg_constraint_create(fsmg_handle h, const fsmg_constraint_config* c, fsmg_constraint* out);
int fsmg_constraint_destroy(fsmg_handle h, fsmg_constraint con);
/* out = { V1, S, C, K } */
int fsmg_constraint_info(fsmg_handle h, fsmg_constraint con, int64_t out[4]);
/* fsmg_generate_filtered under constraint con (NULL: fsmg_generate_filtered itself) */
int fsmg_generate_constrained(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, fsmg_constraint con,
                              fsmg_constraint_state* cstate_io, const int32_t* primer, int32_t* out_tokens, float* out_logprob);
/* fsmg_dstate_generate (below) under constraint con: the caller carries cstate_io from call to call, the decode state itself holds
 * no constraint state */
int fsmg_dstate_generate_constrained(fsmg_handle h, struct fsmg_dstate_s* st, const fsmg_gen_config* g, const fsmg_gen_filters* f,
                                     fsmg_constraint con, fsmg_constraint_state* cstate_io, int32_t* out_tokens,
                                     float* out_logprob);
/* fsmg_maml_generate_filtered (support_len == NULL) or fsmg_maml_generate_filtered_masked: adapt, generate at theta' under con,
 * restore theta */
int fsmg_maml_generate_constrained(fsmg_handle h, const fsmg_gen_config* g, const fsmg_gen_filters* f, fsmg_constraint con,
                                   fsmg_constraint_state* cstate_io, const int32_t* support, const int32_t* support_len,
                                   int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                   const int32_t* primer, int32_t* out_tokens, float* out_logprob);

/* ---- batched on-device beam search (DESIGN.md "Beam search").  G independent searches of width W.  Every hypothesis of group g
 * reads [start, primer[g][0..P-1], y_0, y_1, ...] from a zero state, exactly as a row of fsmg_generate does, and the logits are
 * fsmg_generate's (all V1 = input_size + 1 columns).  At generated position t, slot j of a group and column v give
 *   lp = fl(logit_v - lse_j)   (lse_j the logsumexp fsmg_generate's log-probs use, bitwise the same number)
 *   s  = fl(cum_j + lp)        (cum_j the slot's score so far: 0 for slot 0 and -inf for the others at t = 0)
 * and the group's W x V1 candidates are ranked by s descending, then j ascending, then logit descending, then v ascending, a NaN
 * s or logit ranking below -inf (and -0 equal to +0); the W best become the next slots in that order.  No length normalisation,
 * no end token: every hypothesis has num tokens.
 * Outputs: out_tokens[g][w][t], out_scores[g][w] = the final cum, out_logprob[g][w][t] = each token's lp.  A group's hypotheses
 * are best first and distinct, and a score is bitwise the fp32 left-to-right sum of its lps.  W = 1 is fsmg_generate at
 * temperature 0, tokens and log-probs bitwise (for rows with a logit above -inf at every position).  A group's output is bitwise
 * independent of G and of the other groups.
 * fsmg_beam_search changes no handle state, like fsmg_generate.  fsmg_maml_beam_search adapts, searches and restores theta with
 * fsmg_maml_generate's wrapper and the same documented side effects (the gradient buffer and the recurrent-launch counters).
 * Errors: FSMG_ERR_INVALID for a bad config (version, nonzero reserved fields, G < 1, W outside [1, 64] or W > V1^num, num < 1,
 * P < 0, primer_on_device not 0 / 1, G * W * (P + num + 1) > 2^30, G * W > 2^20, null outputs); FSMG_ERR_TOKEN_RANGE for a
 * primer id outside [0, input_size) (outputs left unwritten). */
#define FSMG_BEAM_CONFIG_VERSION 1
typedef struct fsmg_beam_config {
    int32_t version;          /* FSMG_BEAM_CONFIG_VERSION                                  */
    int32_t n_groups;         /* G >= 1 independent searches                               */
    int32_t beam_width;       /* W, 1 <= W <= 64, and W <= V1^num                          */
    int32_t num;              /* tokens generated per hypothesis, >= 1                     */
    int32_t primer_len;       /* P >= 0 primer tokens per GROUP (shared by its W beams)    */
    int32_t primer_on_device; /* 0 host, 1 device                                          */
    int32_t reserved[8];      /* must be 0                                                 */
} fsmg_beam_config;

/* primer [G,P] (NULL if P == 0); out_tokens host [G,W,num]; out_scores host [G,W]; out_logprob host [G,W,num] or NULL */
int fsmg_beam_search(fsmg_handle h, const fsmg_beam_config* b, const int32_t* primer,
                     int32_t* out_tokens, float* out_scores, float* out_logprob);
/* adapt on support [n_support_rows, max_len] like fsmg_maml_generate, search at theta', restore theta */
int fsmg_maml_beam_search(fsmg_handle h, const fsmg_beam_config* b, const int32_t* support, int32_t n_support_rows,
                          int32_t inner_steps, float inner_lr, int32_t support_on_device, const int32_t* primer,
                          int32_t* out_tokens, float* out_scores, float* out_logprob);
/* fsmg_maml_beam_search with per-song support lengths: support_len as in fsmg_maml_generate_filtered_masked (same checks, same
 * errors); the search at theta' is fsmg_maml_beam_search's */
int fsmg_maml_beam_search_masked(fsmg_handle h, const fsmg_beam_config* b, const int32_t* support, const int32_t* support_len,
                                 int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                                 const int32_t* primer, int32_t* out_tokens, float* out_scores, float* out_logprob);

/* ---- constrained beam search: fsmg_beam_search ranked over the allowed set of a constraint (above), every slot
 * carrying a constraint state.  Everything in fsmg_beam_search's contract holds except what is stated here.
 * Slot state.  Every slot of every group carries (state, open[ceil(K / 32)], dead_ends).  A group's W slots start from the group's
 * state: cstate_in[g] (NULL, or a NULL array: start_state, every slot closed, zero dead ends), walked over the group's primer tokens
 * exactly as fsmg_generate_constrained walks a row's primer, with the same refusals (a host primer token that is not allowed where it
 * stands: FSMG_ERR_INVALID before any device work, before the adaptation in the MAML variant; a device primer: the primer flag,
 * FSMG_ERR_TOKEN_RANGE, outputs unwritten).
 * Candidates.  At a generated position slot j has state (s, open), raw logits z and lse_j, bitwise fsmg_beam_search's number.  With
 * Omega_j the allowed set of (s, open):
 *   Omega_j not empty: the slot's candidates are the columns of Omega_j only, z^c_v = fl(z_v + bias_v), lp = fl(z^c_v - lse_j),
 *     s = fl(cum_j + lp).  A column outside Omega_j is no candidate at all (not one with score -inf: it ranks below an allowed
 *     column whose z^c is -inf or NaN); a slot with |Omega_j| < W has fewer candidates.
 *   Omega_j empty (a dead end): the slot's candidates are all V1 columns with z^c = z, as fsmg_beam_search produces them; they
 *     form a lower tier.
 * Ranking within a group: slots that are not at a dead end first; then s descending; j ascending; z^c descending; v ascending (NaN
 * below -inf, -0 equal to +0).  The W best become the next slots.  A live slot always has at least one candidate and a dead-end
 * slot min(W, V1), so a group always has at least W.
 * Advance.  A winner from a live slot takes its parent's state advanced by its token (next_state, the slot bit flipped); one from
 * a dead-end slot takes its parent's state unchanged with dead_ends + 1, so a dead-end state stays one.  A group's output is
 * therefore its hypotheses with no dead end during the call, best first, followed by those that hit one.  A dead-end hypothesis
 * survives only while its group has fewer than W candidates from live slots; -inf-scored duplicates of live slots count as such
 * candidates, exactly as slots 1 .. W-1 count at the first position of fsmg_beam_search.
 * Outputs.  out_logprob is lp as ranked (the biased value; where the bias is 0 the model's log-prob); out_scores the final cum,
 * bitwise the fp32 left-to-right sum of the hypothesis's out_logprob; hypotheses with a score above -inf are distinct.  cstate_out
 * (may be NULL, as may each of its arrays) receives the final state per hypothesis: state [G*W], open [G*W][ceil(K / 32)],
 * dead_ends [G*W].  cstate_in is per group: state [G], open [G][ceil(K / 32)], dead_ends [G].
 * con == NULL: the call is bitwise fsmg_beam_search (fsmg_dstate_beam_search, fsmg_maml_beam_search(_masked)) on the same kernels;
 * neither state struct is touched.
 * W = 1: the tokens and final constraint states are fsmg_generate_constrained's at temperature 0 with no filters, and the log-probs
 * are equal as floats when every bias value is 0 or -inf (for rows without NaN logits).
 * Errors: what fsmg_beam_search and fsmg_generate_constrained refuse: a constraint this handle does not own, a cstate_in state
 * outside [0, S), negative dead_ends, an open bit at or above K.  Nothing on the handle changes; the MAML variant has
 * fsmg_maml_beam_search's documented side effects only.  Not covered: length normalisation and end tokens (as fsmg_beam_search). */
int fsmg_beam_search_constrained(fsmg_handle h, const fsmg_beam_config* b, fsmg_constraint con, const fsmg_constraint_state* cstate_in,
                                 fsmg_constraint_state* cstate_out, const int32_t* primer, int32_t* out_tokens, float* out_scores,
                                 float* out_logprob);
/* fsmg_dstate_beam_search (below) under con: cstate_in is the groups' constraint state behind what the decode state has read; the
 * decode state is only read */
int fsmg_dstate_beam_search_constrained(fsmg_handle h, struct fsmg_dstate_s* st, const fsmg_beam_config* b, fsmg_constraint con,
                                        const fsmg_constraint_state* cstate_in, fsmg_constraint_state* cstate_out,
                                        int32_t* out_tokens, float* out_scores, float* out_logprob);
/* fsmg_maml_beam_search (support_len == NULL) or fsmg_maml_beam_search_masked: adapt, search at theta' under con, restore theta */
int fsmg_maml_beam_search_constrained(fsmg_handle h, const fsmg_beam_config* b, fsmg_constraint con,
                                      const fsmg_constraint_state* cstate_in, fsmg_constraint_state* cstate_out,
                                      const int32_t* support, const int32_t* support_len, int32_t n_support_rows, int32_t inner_steps,
                                      float inner_lr, int32_t support_on_device, const int32_t* primer, int32_t* out_tokens,
                                      float* out_scores, float* out_logprob);

/* ---- scoring of given songs (DESIGN.md "Scoring").  Row r of tokens [R, max_len] is read exactly as an eval row: the inputs are
 * [start, x_0 .. x_{T-2}] (start = input_size, T = max_len) from a zero state, z the V1 = input_size + 1 logits after input t -- the
 * numbers a training forward pass puts in row t * B + b of its logits -- and y = x_t the target.  Per position:
 *   out_logprob[r][t] = fl(z_y - lse), lse = m + log(sum_v exp(z_v - m)), m the row maximum: the untempered model log-probability,
 *                       the quantity fsmg_generate reports for its own tokens;
 *   out_rank[r][t]    = #{v : z_v > z_y} + #{v < y : z_v == z_y}: 0-based, the lower index first on ties (the decode driver's rule);
 *   out_entropy[r][t] = lse - sum_v p_v z_v, p_v = exp(z_v - lse); a column with z_v = -inf contributes 0, not NaN;
 *   out_argmax[r][t]  = the lowest index holding the row maximum;
 * and per row, with t0 = nll_first and t1 = nll_count ? t0 + nll_count : T (a continuation scored without its primer):
 *   out_row_nll[r]    = -(sum of out_logprob[r][t], t0 <= t < t1) / (t1 - t0), accumulated in fp64 in increasing t and rounded once
 *                       to fp32: bitwise recomputable from out_logprob.
 * A row with a NaN logit gives NaN log-prob and entropy; its rank and argmax are unspecified but in [0, V1); the call succeeds.
 * Passes: the R rows are processed pass_rows at a time, the last pass shorter.  The outputs are bitwise those of scoring each pass's
 * rows in a call of their own; the pass size is a function of the config alone, never of what the handle ran before; two identical
 * calls give identical bits.  A row's bits are NOT promised independent of its pass's row count (the recurrent kernel family and
 * the projection's kernel follow the rows).  Any output may be NULL (not all): the others keep their bits.
 * State: parameters, Adam moments, global_step, the loss ring and the gradient buffer are untouched by fsmg_score; activations
 * (fsmg_debug_read) are overwritten -- "logits" then holds the last pass's logits, time-major --; the recurrent-launch counters of
 * fsmg_stats advance as in fsmg_eval_batch, and a time-out of a persistent recurrent kernel is handled as there (the pass is
 * repeated on per-step launches).  fsmg_maml_score adapts like fsmg_maml_eval, scores at theta' and restores theta whatever
 * happens: exactly fsmg_maml_generate's documented side effects (the gradient buffer, the recurrent-launch counters).
 * Errors: FSMG_ERR_INVALID for a wrong version, nonzero reserved fields, n_rows < 1 (or > 2^20), tokens_on_device not 0 / 1,
 * nll_first outside [0, T) or nll_first + nll_count > T or nll_count < 0, pass_rows outside {0} u [1, 1024], every output NULL, NULL
 * tokens; FSMG_ERR_TOKEN_RANGE for a token outside [0, input_size).  After an error the contents of the outputs are unspecified. */
#define FSMG_SCORE_CONFIG_VERSION 1
#define FSMG_SCORE_PASS_ROWS 128          /* default rows per device pass */
typedef struct fsmg_score_config {
    int32_t version;          /* FSMG_SCORE_CONFIG_VERSION                                   */
    int32_t n_rows;           /* R >= 1 songs of max_len tokens each                         */
    int32_t tokens_on_device; /* 0 host, 1 device                                            */
    int32_t nll_first;        /* t0 in [0, T): first position counted in out_row_nll         */
    int32_t nll_count;        /* 0 = up to T, else t0 + nll_count <= T                       */
    int32_t pass_rows;        /* 0 = FSMG_SCORE_PASS_ROWS, else 1..1024                      */
    int32_t reserved[10];     /* must be 0                                                   */
} fsmg_score_config;

/* tokens [R,T]; host outputs, any may be NULL but not all:
   out_logprob [R,T], out_rank [R,T], out_entropy [R,T], out_argmax [R,T], out_row_nll [R] */
int fsmg_score(fsmg_handle h, const fsmg_score_config* c, const int32_t* tokens,
               float* out_logprob, int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll);
/* adapt on support [n_support_rows, max_len] like fsmg_maml_generate, score at theta', restore theta */
int fsmg_maml_score(fsmg_handle h, const fsmg_score_config* c, const int32_t* support, int32_t n_support_rows,
                    int32_t inner_steps, float inner_lr, int32_t support_on_device, const int32_t* tokens,
                    float* out_logprob, int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll);
/* fsmg_maml_score with per-song support lengths: support_len as in fsmg_maml_generate_filtered_masked (same checks, same errors).
 * lengths (host [R], every one in [1, max_len]; NULL: fsmg_maml_score's outputs) are the SCORED songs' own and shape the outputs as
 * fsmg_score_masked does: 0 behind a song's end, out_row_nll over the positions inside the song. */
int fsmg_maml_score_masked(fsmg_handle h, const fsmg_score_config* c, const int32_t* support, const int32_t* support_len,
                           int32_t n_support_rows, int32_t inner_steps, float inner_lr, int32_t support_on_device,
                           const int32_t* tokens, const int32_t* lengths, float* out_logprob, int32_t* out_rank,
                           float* out_entropy, int32_t* out_argmax, float* out_row_nll);

/* ---- decode states (DESIGN.md "Decode states"): the LSTM state of R decode rows as a device-resident object the handle owns, so
 * that every decode entry point can start from it and leave it advanced -- continue a piece, read something longer than max_len in
 * chunks, read an artist's support songs and go on from there.  The one-shot entry points above start every row from a zero state
 * and throw the state away; they are unchanged.
 * A state holds, per row: h and c of every layer; a PENDING token, the next input the cells read; the last `history` context tokens.
 * And for all rows together (the rows of a state advance in lockstep): n_ctx, the number of context tokens so far, and n_gen, how
 * many of them were generated.  A fresh (created or reset) state has zero h and c, n_ctx = n_gen = 0 and the start word
 * (input_size) pending; that implicit start word is not context, as in fsmg_generate_filtered.
 *   fsmg_dstate_feed      given tokens x_0 .. x_{n-1} per row ([R][n]; ids in [0, input_size]: the start word may be fed explicitly,
 *                         which is how a new song is begun on a carried state, and an explicitly fed start word IS context).  For each
 *                         x_i in order: the pending token is read through the cells; with out_logprob != NULL,
 *                         out_logprob[r][i] = fl(z[x_i] - lse) from that output, z the V1 logits fsmg_generate computes and lse
 *                         bitwise the number its log-probs use; then x_i becomes pending and joins the context.  Without
 *                         out_logprob no logits are computed (the cells-only primer path).  n_ctx += n.
 *   fsmg_dstate_generate  at local position t the pending token is read and a token picked exactly as fsmg_generate_filtered picks
 *                         it (g->n_seq == rows, g->primer_len == 0), with Philox counter (v >> 2, n_gen + t, b, 0), b the row index in
 *                         the state; the token becomes pending and joins the context; n_ctx += num, n_gen += num.  The repetition
 *                         penalty's context is the last min(repeat_window, n_ctx + t) tokens of (the history followed by this
 *                         call's tokens): with a penalty on, repeat_window must be in [1, history], and repeat_window = 0 (the
 *                         whole context) is allowed only while n_ctx + num <= history.
 *   fsmg_dstate_beam_search  group g starts from state row g with beam_width copies of it (b->n_groups == rows, b->primer_len == 0);
 *                         the state is read and not modified.
 * What follows from it, all bitwise: a fresh state, feed(primer) without log-probs, generate(num) gives
 * fsmg_generate_filtered(primer, num) with the same config, seed and filters, tokens and log-probs (with a penalty: while its window
 * fits the history); generate(a) then generate(b) gives generate(a + b); feed(x[:a]) then feed(x[a:]) gives feed(x); the log-probs
 * feed returns for tokens generate produced are the ones generate reported; a row's outputs depend neither on the row count nor on
 * the other rows; fresh state, feed(primer), beam_search gives fsmg_beam_search(primer); get followed by set into a fresh state of
 * the same shape continues with the same bits.  No other handle state changes (fsmg_generate's list), and the one-shot entry points
 * return the bits they returned before states existed.
 *   fsmg_dstate_create / _destroy  a state of n_rows rows keeping `history` context tokens; its storage is its own allocation.
 *                         fsmg_destroy frees the states still alive.
 *   fsmg_dstate_reset     back to the fresh state.
 *   fsmg_dstate_info      out = {rows, history, n_ctx, n_gen}.
 *   fsmg_dstate_get       h_out / c_out host [L][R][H] (the reference's layout: H, not the padded width), ctx_out host
 *                         [R][min(n_ctx, history)] oldest first (its last token is the pending one); any may be NULL.
 *   fsmg_dstate_set       the reverse (pad units are written as zero; n_gen <= n_ctx; ctx_in may be NULL when n_ctx = 0, and then
 *                         the start word is pending).
 *   fsmg_dstate_gather    dst row i = src row rows[i] (host indices, repeats allowed; dst->rows of them), equal history, dst != src;
 *                         the counters are copied.
 * Errors: FSMG_ERR_INVALID for a state this handle does not own or one already destroyed (the handle keeps a registry: an error,
 * not a crash), a wrong version or nonzero reserved fields, n_rows < 1 (or > 2^20), history < 1, a row-count mismatch, a primer_len
 * other than 0, a gather index out of range, the window rules above, n < 0, tokens_on_device not 0 / 1, rows * (history + n + 1) >
 * 2^30 (n = the call's tokens), n_gen + num > 2^31 - 1, and everything fsmg_generate_filtered / fsmg_beam_search refuse;
 * FSMG_ERR_TOKEN_RANGE for a fed id or a ctx_in id outside [0, input_size].  Host tokens are checked before any device work; device
 * tokens by a flag read back with the outputs.  An argument error leaves the state untouched; after a token-range error on DEVICE
 * tokens the state's contents are unspecified (reset it or set it).
 * States at MAML's theta' do not exist: a state would outlive the restored parameters. */
#define FSMG_DSTATE_CONFIG_VERSION 1
typedef struct fsmg_dstate_s* fsmg_dstate;
typedef struct fsmg_dstate_config {
    int32_t version;          /* FSMG_DSTATE_CONFIG_VERSION                                  */
    int32_t n_rows;           /* R >= 1 rows advancing in lockstep                           */
    int32_t history;          /* >= 1 context tokens kept per row (the penalty's reach)      */
    int32_t reserved[9];      /* must be 0                                                   */
} fsmg_dstate_config;

int fsmg_dstate_create(fsmg_handle h, const fsmg_dstate_config* c, fsmg_dstate* out);
int fsmg_dstate_destroy(fsmg_handle h, fsmg_dstate st);
int fsmg_dstate_reset(fsmg_handle h, fsmg_dstate st);
int fsmg_dstate_info(fsmg_handle h, fsmg_dstate st, int64_t out[4]);
int fsmg_dstate_get(fsmg_handle h, fsmg_dstate st, float* h_out, float* c_out, int32_t* ctx_out);
int fsmg_dstate_set(fsmg_handle h, fsmg_dstate st, const float* h_in, const float* c_in, const int32_t* ctx_in, int64_t n_ctx,
                    int64_t n_gen);
int fsmg_dstate_gather(fsmg_handle h, fsmg_dstate dst, fsmg_dstate src, const int32_t* rows);
/* tokens [R,n] host, or device when tokens_on_device; out_logprob host [R,n] or NULL */
int fsmg_dstate_feed(fsmg_handle h, fsmg_dstate st, const int32_t* tokens, int32_t n, int32_t tokens_on_device, float* out_logprob);
/* out_tokens host [R,num], out_logprob host [R,num] or NULL; f may be NULL */
int fsmg_dstate_generate(fsmg_handle h, fsmg_dstate st, const fsmg_gen_config* g, const fsmg_gen_filters* f, int32_t* out_tokens,
                         float* out_logprob);
/* out_tokens host [R,W,num]; out_scores host [R,W]; out_logprob host [R,W,num] or NULL */
int fsmg_dstate_beam_search(fsmg_handle h, fsmg_dstate st, const fsmg_beam_config* b, int32_t* out_tokens, float* out_scores,
                            float* out_logprob);

/* ---- support-set neural cache (DESIGN.md "Support-set cache"; Grave, Joulin, Usunier: Improving neural language models with a
 * continuous cache).  The few-shot route that needs no gradient: keep the top-layer hidden states the model produced while reading an
 * artist's support songs, each with the token that followed it; at a query position attend over them with the query's own hidden
 * state; mix the resulting distribution with the model's.
 * A cache is a device-resident object the handle owns: G groups (one per artist) of Mg entries each; an entry is a key of H floats
 * (stored padded, the pad units exact zeros) and an int32 value, the token that followed.  A cache is DATA: it holds vectors and does
 * not refer to the parameters.  It stays valid -- and STALE -- after a train step, fsmg_set_param or fsmg_init_params: it still holds
 * the vectors of the parameters it was built with, and scoring against it is defined and deterministic.  Caches at MAML's theta' do
 * not exist.
 *   fsmg_cache_build      rows tokens [n_rows, max_len], read exactly as fsmg_score reads a row; row r belongs to group
 *                         r / (n_rows / n_groups).  Entry e = (r mod rows_per_group) * T + t of that group: the key is the top-layer h
 *                         after the inputs [start, x_0 .. x_{t-1}] -- the vector whose projection is the logits row fsmg_score scores
 *                         at (r, t) -- and the value is x_t.  Mg = (n_rows / n_groups) * T.  No logits are computed.  The rows are
 *                         processed pass_rows at a time, the last pass shorter; the keys are bitwise the top-layer hidden states an
 *                         fsmg_score pass over the same rows with the same pass_rows computes; the cache is bitwise what building each
 *                         pass's rows in a call of their own gives; the pass size is a function of the config alone; two identical
 *                         calls give identical bits.  A row's bits are NOT promised independent of its pass's row count.
 *                         State: exactly fsmg_score's -- parameters, Adam moments, global_step, the loss ring and the gradient buffer
 *                         untouched, activations overwritten, the recurrent-launch counters advance, a time-out of a persistent
 *                         recurrent kernel repeats the pass on per-step launches.
 *   fsmg_cache_create_from  a cache from host arrays: keys [G][Mg][H], values [G][Mg] (ids in [0, input_size]).
 *   fsmg_cache_get        the reverse; either output may be NULL.
 *   fsmg_cache_info       out = {groups, entries per group, H, device bytes}.
 *   fsmg_cache_destroy    frees it; fsmg_destroy frees the caches still alive.
 *   fsmg_cache_attend     for query vector q (host [n][H]) in group g (host [n], NULL = all 0) with target y and sharpness theta >= 0:
 *                           d_i = q . k_i over the group's Mg keys (exact products of the fp32 inputs, fp64 accumulation),
 *                           p_cache(y) = sum_{i : v_i = y} exp(theta (d_i - d_max)) / sum_i exp(theta (d_i - d_max)),
 *                         exactly 0 when no entry holds y; out_prob host [n_theta][n].  Deterministic (no atomics); a query's bits
 *                         depend on its vector, its group's entries and theta alone -- not on the other queries of the call, their
 *                         number or the query's place among them.
 *   fsmg_cache_score      fsmg_score's rows with the cache beside the model: per pass the model log-prob lp (fsmg_score's kernel) and
 *                         p_cache(y) for the pass's own top-layer hidden states as queries (no host round trip), row r in group
 *                         group[r] (host [R], NULL = all 0).  Outputs, any may be NULL but not all:
 *                           out_lstm_logprob [R][T]                  bitwise fsmg_score's out_logprob for the same rows and pass_rows;
 *                           out_cache_prob   [n_theta][R][T]         p_cache(y), bitwise fsmg_cache_attend on the pass's hidden states;
 *                           out_logprob      [n_theta][n_lambda][R][T]  log((1 - lambda) exp(lp) + lambda p_cache), evaluated on the
 *                                            host in fp64 from the two fp32 numbers and rounded once: a = log1p(-lambda) + lp,
 *                                            b = log(lambda) + log(p_cache) (-inf at p_cache = 0), out = logaddexp(a, b); lambda = 0
 *                                            gives lp bitwise, lambda = 1 gives log(p_cache);
 *                           out_row_nll      [n_theta][n_lambda][R]  fsmg_score's definition over out_logprob (nll_first / nll_count):
 *                                            an fp64 sum in increasing t, rounded once; bitwise recomputable from out_logprob.
 *                         The whole (theta, lambda) grid costs one device pass.  Passes, state and time-outs as fsmg_score.
 *   fsmg_cache_eval_step  support [N,K,T] and query [N,Q,T] on the host: builds a cache of N groups of K rows, scores the N * Q query
 *                         rows with group = artist, *nll = -(fp64 mean of out_logprob), destroys the cache.  fsmg_eval_step's number
 *                         with the support set used instead of ignored; lambda = 0 gives the model's own NLL.
 * Errors: FSMG_ERR_INVALID for a cache this handle does not own or one already destroyed (a registry: an error, not a crash), a wrong
 * version, nonzero reserved fields, n_rows < 1 (or > 2^20), n_groups < 1, n_rows not a multiple of n_groups, tokens_on_device not
 * 0 / 1, pass_rows outside {0} u [1, 1024], the nll window rules of fsmg_score, n_theta outside [1, 8], a theta that is negative or not
 * finite, n_lambda outside [1, 16], a lambda outside [0, 1], n < 1 (or > 2^22), a group id outside [0, G), a cache whose H is not the
 * handle's, every output NULL, NULL arguments, G < 1, Mg < 1, G * Mg > 2^22, G * Mg * Hp * 4 > 2^31 (Hp the padded hidden size);
 * FSMG_ERR_TOKEN_RANGE for a token outside [0, input_size) or a value outside [0, input_size].  Host tokens are checked before any
 * device work. */
#define FSMG_CACHE_CONFIG_VERSION 1
#define FSMG_CACHE_SCORE_CONFIG_VERSION 1
#define FSMG_CACHE_MAX_THETA 8
#define FSMG_CACHE_MAX_LAMBDA 16
typedef struct fsmg_cache_s* fsmg_cache;
typedef struct fsmg_cache_config {
    int32_t version;          /* FSMG_CACHE_CONFIG_VERSION                                   */
    int32_t n_rows;           /* support rows of max_len tokens each                         */
    int32_t n_groups;         /* G >= 1; n_rows % n_groups == 0                              */
    int32_t tokens_on_device; /* 0 host, 1 device                                            */
    int32_t pass_rows;        /* 0 = FSMG_SCORE_PASS_ROWS, else 1..1024                      */
    int32_t reserved[11];     /* must be 0                                                   */
} fsmg_cache_config;
typedef struct fsmg_cache_score_config {
    int32_t version;          /* FSMG_CACHE_SCORE_CONFIG_VERSION                             */
    int32_t n_rows;           /* R >= 1 songs of max_len tokens each                         */
    int32_t tokens_on_device; /* 0 host, 1 device                                            */
    int32_t nll_first;        /* as fsmg_score_config                                        */
    int32_t nll_count;        /* as fsmg_score_config                                        */
    int32_t pass_rows;        /* 0 = FSMG_SCORE_PASS_ROWS, else 1..1024                      */
    int32_t n_theta;          /* 1..8                                                        */
    int32_t n_lambda;         /* 1..16                                                       */
    float thetas[8];          /* finite, >= 0; the first n_theta count                       */
    float lambdas[16];        /* in [0, 1]; the first n_lambda count                         */
    int32_t reserved[8];      /* must be 0                                                   */
} fsmg_cache_score_config;

int fsmg_cache_build(fsmg_handle h, const fsmg_cache_config* c, const int32_t* tokens, fsmg_cache* out);
/* keys host [G][Mg][H], values host [G][Mg] */
int fsmg_cache_create_from(fsmg_handle h, int32_t n_groups, int32_t entries_per_group, const float* keys, const int32_t* values,
                           fsmg_cache* out);
int fsmg_cache_get(fsmg_handle h, fsmg_cache cache, float* keys, int32_t* values);
int fsmg_cache_info(fsmg_handle h, fsmg_cache cache, int64_t out[4]);
int fsmg_cache_destroy(fsmg_handle h, fsmg_cache cache);
/* queries host [n][H], targets host [n], group host [n] or NULL, thetas host [n_theta], out_prob host [n_theta][n] */
int fsmg_cache_attend(fsmg_handle h, fsmg_cache cache, int32_t n, const float* queries, const int32_t* targets, const int32_t* group,
                      const float* thetas, int32_t n_theta, float* out_prob);
/* tokens [R,T]; group host [R] or NULL; host outputs, any may be NULL but not all */
int fsmg_cache_score(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const int32_t* tokens, const int32_t* group,
                     float* out_logprob, float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll);
int fsmg_cache_eval_step(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q, float theta,
                         float lambda, float* nll);

/* ---- cache-conditioned generation (DESIGN.md "Cache-conditioned generation").  fsmg_generate_filtered with a support-set cache beside
 * the model: at every GENERATED position each row's next token is drawn from the mixture fsmg_cache_score scores,
 * p = (1 - lambda) p_lstm + lambda p_cache, the row attending over group group[r] of the cache (host [n_seq], NULL = all 0) with its
 * own top-layer hidden state -- the vector whose projection is the position's logits row -- as the query.  On the device, per row:
 *   d_i = q . k_i over the group's Mg keys (fsmg_cache_attend's arithmetic: exact products of the fp32 inputs, fp64 accumulation in a
 *   fixed order), w_i = exp(theta (d_i - d_max)), Z = sum_i w_i, p_cache(v) = fl32((sum_{i : v_i = v} w_i) / Z), exactly 0 for a v no
 *   entry holds; lp_v = fl32(z_v - lse), lse bitwise the number fsmg_generate subtracts for its log-probs;
 *   z''_v = fl32(logaddexp(log1p(-lambda) + lp_v, log(lambda) + log(p_cache(v)))) in fp64 from the two fp32 numbers (fsmg_cache_score's
 *   out_logprob formula); fl32(log1p(-lambda) + lp_v) where p_cache(v) = 0, which is -inf at lambda = 1.
 * The unchanged pick of fsmg_generate(_filtered) then reads z'' as if it were the logits row: temperature, top_k, the filters, the
 * Philox counters and the tie rules are fsmg_generate's, and out_logprob is what that pick reports on z'': z''_tok - lse(z''), with
 * lse(z'') = 0 up to rounding.  Primer positions run the cells only: the cache is read at generated positions only.
 *   fsmg_cache_generate         fsmg_generate_filtered's arguments and outputs.  lambda = 0: the cache is not read at all, and tokens and
 *                               log-probs are fsmg_generate_filtered's BITWISE.
 *   fsmg_dstate_cache_generate  fsmg_dstate_generate likewise (lambda = 0: its bits): from a decode state and back into it.  With the
 *                               same cache and config its composition laws hold bitwise: generate(a) then generate(b) equals
 *                               generate(a + b); a fresh state, fsmg_dstate_feed(primer), generate equals the one-shot call.
 *   fsmg_cache_distribution     the kernels on given vectors: queries host [n][H], logits host [n][V1] (V1 = input_size + 1), group host
 *                               [n] or NULL.  Outputs, any may be NULL but not all: out_cache_prob [n][V1] (p_cache), out_logprob [n][V1]
 *                               (z''), out_lse [n] (lse).  lambda = 0 still returns out_cache_prob, and out_logprob = lp bitwise.
 * Everything fsmg_generate promises holds: two identical calls give identical bits; a row's tokens and log-probs depend on its own
 * primer, row index, group and that group's entries, the config and the seed -- not on n_seq, the other rows or their groups; no
 * handle state is changed (the cache gains a value index -- its entries in stable order by value -- on the first call with lambda > 0
 * or the first fsmg_cache_distribution: fsmg_cache_info's byte count grows once, fsmg_cache_get / _attend / _score keep their bits).
 * A row's z'' bits in fsmg_cache_distribution depend on its query, its logits row, its group's entries, theta and lambda alone.
 * A stale cache is legal, as for fsmg_cache_score.  The keys of a call are walked in chunks of FSMG_CACHE_GEN_CHUNK entries, one
 * wave each; no result depends on it.
 * Errors: FSMG_ERR_INVALID for a cache (or state) this handle does not own or one already destroyed, a cache whose H is not the
 * handle's, a wrong version, nonzero reserved words, theta negative or not finite, lambda outside [0, 1] or NaN, a group id outside
 * [0, G), n < 1 or n > 2^20, rows * Mg > 2^26 (the fp64 score scratch), every output NULL, NULL queries / logits, and everything
 * fsmg_generate_filtered / fsmg_dstate_generate refuse; FSMG_ERR_TOKEN_RANGE as they return it.  Argument errors are found before any
 * device work: outputs and states are untouched.
 * Out of scope: beam search over the mixture; the row's own history in the set (fsmg_cache_self_generate has it); caches or states
 * at MAML's theta'; several thetas per call. */
#define FSMG_CACHE_GEN_CONFIG_VERSION 1
#define FSMG_CACHE_GEN_CHUNK 16
typedef struct fsmg_cache_gen_config {
    int32_t version;      /* FSMG_CACHE_GEN_CONFIG_VERSION                               */
    float   theta;        /* finite, >= 0                                                */
    float   lambda;       /* in [0, 1]; 0: the cache is not read at all                  */
    int32_t reserved[13]; /* must be 0                                                   */
} fsmg_cache_gen_config;

/* fsmg_generate_filtered with the cache beside the model; group host [n_seq] or NULL (all 0) */
int fsmg_cache_generate(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_gen_config* g,
                        const fsmg_gen_filters* f, const int32_t* group, const int32_t* primer,
                        int32_t* out_tokens, float* out_logprob);
/* fsmg_dstate_generate likewise: from a carried state and back into it */
int fsmg_dstate_cache_generate(fsmg_handle h, fsmg_dstate st, fsmg_cache cache, const fsmg_cache_gen_config* cc,
                               const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* group,
                               int32_t* out_tokens, float* out_logprob);
/* the kernels on given vectors: queries host [n][H], logits host [n][V1], group host [n] or NULL;
   outputs, any may be NULL but not all: out_cache_prob [n][V1], out_logprob [n][V1] (z''), out_lse [n] */
int fsmg_cache_distribution(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, int32_t n, const float* queries,
                            const float* logits, const int32_t* group, float* out_cache_prob, float* out_logprob, float* out_lse);

/* ---- self-cache (DESIGN.md "Self-cache"): the continuous cache of Grave, Joulin and Usunier over the sequence's OWN history.  It
 * needs no support set; with one, the own entries join the group's entries in ONE softmax.
 * A row is read exactly as fsmg_score reads it: the inputs are [start, x_0 .. x_{T-2}], q_t is the top-layer h after input t (the
 * vector whose projection is the logits row at t), the target is y_t = x_t.
 *   own entries  own entry i of a row is (key = q_i, value = x_i): the entry fsmg_cache_build would file for that row at position i.
 *   window       with window W >= 1, position t sees its own entries max(0, t - W) .. t - 1.  Strictly causal: entry t itself, whose
 *                value is the target, is never visible.
 *   union        with a support cache the row's group's Mg entries are added; one softmax over the union, one theta, one lambda:
 *                  d_i = q_t . k_i,  p_cache(y) = sum_{i in set, v_i = y} exp(theta (d_i - d_max)) / sum_{i in set} exp(theta (d_i - d_max)),
 *                exactly 0 when no visible entry holds y.
 *   empty set    no support cache and t = 0: the position is scored by the model alone: p_cache = 0 and the mixed log-prob is lp
 *                BITWISE at every lambda, lambda = 1 included (no mixture that normalises exists there).
 *   arithmetic   fsmg_cache_attend's: fp32 inputs widened exactly, exact products, fp64 accumulation in a fixed k order; the exponent
 *                in fp64 up to the last step with integer shifts ceil(u m); fp64 sums in an order that depends on Mg, t and W alone;
 *                no atomics.  The pad units of an own key contribute exact zeros whatever the pass left in them.
 *   fsmg_cache_self_score   fsmg_cache_score's arguments, outputs, passes, state rules and time-out retry, with the own entries in
 *                           the set; cache == NULL is the pure self-cache (group is then ignored).  out_lstm_logprob is bitwise
 *                           fsmg_score's; out_logprob is fsmg_cache_score's host formula over the two device outputs, except at an
 *                           empty-set position (above); the whole (theta, lambda) grid costs one device pass.
 *   fsmg_cache_self_attend  the scoring kernel on given vectors: vectors host [n_rows][n_pos][H], values host [n_rows][n_pos] (ids in
 *                           [0, input_size]): values[r][t] is both the target of position t and the value of own entry t; group host
 *                           [n_rows] or NULL (all 0; ignored without a cache); out_prob host [n_theta][n_rows][n_pos].
 * Two identical calls give identical bits.  A position's bits depend on its row's vectors and values 0 .. t, its group's entries,
 * theta and W alone: not on the number of rows of the call or pass, nor on the other rows.  fsmg_cache_score / _attend / _get and
 * fsmg_cache_generate keep their bits; the cache is not changed.
 * Errors: FSMG_ERR_INVALID for everything fsmg_cache_score / fsmg_cache_attend refuse, a NULL or wrongly versioned
 * fsmg_cache_self_config, nonzero reserved words, window < 1, n_rows < 1, n_pos < 1, n_rows * n_pos > 2^22; FSMG_ERR_TOKEN_RANGE for
 * a value outside [0, input_size] (a token outside [0, input_size) in fsmg_cache_self_score).  Argument errors are found before any
 * device work: outputs are untouched.
 * Decode time.  fsmg_cache_self_generate is fsmg_cache_generate (its arguments, outputs, picks, filters, Philox counters and promises)
 * with the row's own history in the set; cache == NULL: the own history alone, group ignored.  Own entry j of a row is (the top
 * layer's h_out when input j of the row's token buffer [start, primer, generated tokens] was read, the token at position j + 1 of
 * that buffer): primer positions are entries too.  At generated position p the visible own entries are max(0, p - W) .. p - 1, in
 * one softmax with the group's support entries: one d_max, one shift, one Z over the union,
 *   p_cache(v) = fl32((support mass of v + own mass of v) / Z),  z'' as fsmg_cache_generate;
 * the own scores have exact fp64 products of the fp32 inputs and fp64 accumulation in one fixed order, the own masses of a value are
 * summed in entry order, no atomics.  An empty union (no cache, p = 0, no primer) leaves the row lp: the model alone.  lambda = 0
 * reads no cache at all and is fsmg_generate_filtered BITWISE.  Two identical calls give identical bits; a row's tokens and
 * log-probs do not depend on n_seq or the other rows; no handle state is changed (a support cache gains its value index once, as
 * for fsmg_cache_generate).
 *   fsmg_cache_self_distribution  the decode-time kernels on given vectors, fsmg_cache_distribution's outputs: queries host [n][H],
 *     logits host [n][V1], self_keys host [n][S][H], self_values host [n][S] (ids in [0, input_size]), self_len host [n], each in
 *     [0, S]: row i sees the LAST min(self_len[i], W) of its first self_len[i] entries.  An empty union gives out_cache_prob 0 and
 *     out_logprob = lp whatever lambda is; lambda = 0 gives lp bitwise.  A row's bits depend on its own inputs alone.
 * Further errors, FSMG_ERR_INVALID: everything fsmg_cache_generate / fsmg_cache_distribution refuse, self_len outside [0, S], S < 0,
 * rows * (primer_len + num) * Hp > 2^29 (the own keys of a call: 2 GiB; Hp the padded hidden size; rows * S * Hp likewise),
 * rows * min(W, primer_len + num) > 2^26 (the fp64 own scores); FSMG_ERR_TOKEN_RANGE for an own value outside [0, input_size].
 * Out of scope: decode-state variants (a state would have to carry keys); beam search over the mixture; separate theta or lambda for
 * own and support entries; anything at MAML's theta'. */
#define FSMG_CACHE_SELF_CONFIG_VERSION 1
typedef struct fsmg_cache_self_config {
    int32_t version;       /* FSMG_CACHE_SELF_CONFIG_VERSION                              */
    int32_t window;        /* W >= 1: a position sees its last min(t, W) own entries      */
    int32_t reserved[14];  /* must be 0                                                   */
} fsmg_cache_self_config;

/* fsmg_cache_score with the row's own history in the set; cache may be NULL */
int fsmg_cache_self_score(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const fsmg_cache_self_config* sc,
                          const int32_t* tokens, const int32_t* group, float* out_logprob, float* out_cache_prob,
                          float* out_lstm_logprob, float* out_row_nll);
/* vectors host [n_rows][n_pos][H], values host [n_rows][n_pos], group host [n_rows] or NULL, out_prob host [n_theta][n_rows][n_pos] */
int fsmg_cache_self_attend(fsmg_handle h, fsmg_cache cache, const fsmg_cache_self_config* sc, int32_t n_rows, int32_t n_pos,
                           const float* vectors, const int32_t* values, const int32_t* group, const float* thetas, int32_t n_theta,
                           float* out_prob);
/* fsmg_cache_generate with the row's own history in the set; cache may be NULL (group is then ignored) */
int fsmg_cache_self_generate(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                             const fsmg_gen_config* g, const fsmg_gen_filters* f, const int32_t* group, const int32_t* primer,
                             int32_t* out_tokens, float* out_logprob);
/* fsmg_cache_distribution over the union: self_keys host [n][S][H], self_values host [n][S], self_len host [n] (each in [0, S]) */
int fsmg_cache_self_distribution(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                                 int32_t n, const float* queries, const float* logits, const float* self_keys, const int32_t* self_values,
                                 const int32_t* self_len, int32_t S, const int32_t* group, float* out_cache_prob, float* out_logprob,
                                 float* out_lse);

/* ---- per-song lengths in scoring and in the support-set cache: ragged groups (DESIGN.md "Ragged cache groups").  Songs are stored
 * zero-padded to max_len; these calls take each row's true length (host int32, every value in [1, max_len]) so that padding is
 * neither scored nor filed as cache entries.  Lengths are checked before any device work; a NULL or out-of-range length gives
 * FSMG_ERR_INVALID with nothing touched.  Position t of row r is SCORED iff t < lengths[r].
 * A RAGGED cache keeps the layout of a uniform one -- G groups of Mg slots, fsmg_cache_info reports Mg, now a capacity -- and adds a
 * per-group entry count n_g in [1, Mg]: entries 0 .. n_g - 1 of group g exist; the slots behind them hold zero keys and value 0, read
 * back as zeros from fsmg_cache_get and are never scored by any kernel (skipped, not scored as a zero key).  Every call that takes a
 * cache (fsmg_cache_attend, _score, _distribution, _generate, fsmg_dstate_cache_generate, fsmg_cache_self_*) accepts a ragged one with
 * no new argument and gives, for group g, bitwise what it gives on a uniform one-group cache made of g's first n_g entries; the
 * size limits (rows * entries_per_group <= 2^26) keep using the capacity Mg.
 *   fsmg_score_masked            fsmg_score with lengths [R]: every per-token output is bitwise fsmg_score's at a scored position (same
 *                                rows, same pass_rows) and +0.0f / 0 behind a song's end; out_row_nll[r] = -(fp64 sum in increasing
 *                                t over nll_first <= t < min(window end, lengths[r])) / (the number of those positions), rounded
 *                                once, bitwise recomputable from out_logprob; NaN when the window holds no scored position.
 *   fsmg_cache_build_masked      fsmg_cache_build with lengths [n_rows]: the same passes (the same hidden states), then position t of
 *                                row r is filed iff t < lengths[r], the entries of a group packed row-major, t increasing, without
 *                                gaps: n_g = the sum of the group's rows' lengths, Mg = (n_rows / n_groups) * max_len.  The tokens
 *                                behind a row's length change no bit of the cache.  Full lengths give fsmg_cache_build's bits.
 *   fsmg_cache_create_from_counts  fsmg_cache_create_from with counts [G], each in [1, Mg]: slots >= counts[g] of keys and values
 *                                are not read (they may hold anything, NaN and out-of-range ids included).
 *   fsmg_cache_counts            out[g] = n_g; Mg for every group of a uniform cache.
 *   fsmg_cache_score_masked      fsmg_cache_score with lengths [R]: outputs bitwise fsmg_cache_score's at scored positions and +0.0f
 *                                behind a song's end; out_row_nll as fsmg_score_masked, per (theta, lambda).  A query behind its
 *                                song's end costs no attention work.
 *   fsmg_cache_self_score_masked the same for fsmg_cache_self_score.
 *   fsmg_cache_eval_step_masked  fsmg_cache_eval_step with support_len [N * K] and query_len [N * Q]: fsmg_cache_build_masked, then
 *                                fsmg_cache_score_masked; *nll = -(fp64 sum, in storage order, of out_logprob over the scored
 *                                positions) / (their number), rounded once.
 * Further errors, FSMG_ERR_INVALID: a count outside [1, entries_per_group], NULL lengths / counts / out. */
int fsmg_score_masked(fsmg_handle h, const fsmg_score_config* c, const int32_t* tokens, const int32_t* lengths, float* out_logprob,
                      int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll);
int fsmg_cache_build_masked(fsmg_handle h, const fsmg_cache_config* c, const int32_t* tokens, const int32_t* lengths, fsmg_cache* out);
/* counts host [G], keys host [G][Mg][H], values host [G][Mg] */
int fsmg_cache_create_from_counts(fsmg_handle h, int32_t n_groups, int32_t entries_per_group, const int32_t* counts, const float* keys,
                                  const int32_t* values, fsmg_cache* out);
int fsmg_cache_counts(fsmg_handle h, fsmg_cache cache, int32_t* out /* [G] */);
int fsmg_cache_score_masked(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const int32_t* tokens,
                            const int32_t* lengths, const int32_t* group, float* out_logprob, float* out_cache_prob,
                            float* out_lstm_logprob, float* out_row_nll);
int fsmg_cache_self_score_masked(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const fsmg_cache_self_config* sc,
                                 const int32_t* tokens, const int32_t* lengths, const int32_t* group, float* out_logprob,
                                 float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll);
int fsmg_cache_eval_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                                const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float theta, float lambda, float* nll);

/* ---- dynamic evaluation (Krause et al., "Dynamic evaluation of neural sequence models", arXiv 1709.07432): the model
 * adapts on the songs it scores.  While it reads a stream of songs it takes a small gradient step on every segment it has just
 * scored, pulled back towards the trained parameters theta by a decay term and, under the RMS rule, scaled per parameter by gradient
 * statistics collected once on training data.  Every reported position is scored BEFORE the model has adapted on it.
 *
 * A stream is an ordered list of n_rows rows `tokens` [n_rows][T] (host int32, one song per row, T = max_len) with optional host
 * `lengths` [n_rows] (NULL: every row has T positions).  Rows [0, first_reported) adapt only; rows [first_reported, n_rows) are
 * reported.  Rows are consumed in blocks: block boundaries stand at every multiple of rows_per_step, at first_reported (a block is
 * never half reported) and at n_rows.  A block of rows is walked in windows [lo, hi) = [i S, min((i + 1) S, T)), S = seg_len,
 * i = 0, 1, ...  theta_l starts as a copy of theta; theta_g is the saved copy of theta.  Per (block, window), with
 * e[b] = min(hi, len[b]) and n_valid = sum_b max(0, e[b] - lo):
 *   1. n_valid == 0: the window is skipped -- no pass, no update.
 *   2. One forward + backward over the block's rows from position 0, zero initial state, at the current theta_l.  Position t of row
 *      b carries the weight fl32(1 / ((double)n_valid + 1e-12)) iff lo <= t < e[b], else an exact 0;
 *      loss = sum of ce over the weighted positions / (n_valid + 1e-12).  Inputs at t < lo are the real tokens (the window's context:
 *      BPTT runs through them); positions t >= e[b] get fixed ids (input: the start word, target: 0), so whatever the caller put
 *      behind a song's end never matters, exactly.
 *   3. A reported block: out_logprob[row][t] = -ce of the weighted positions of this window -- the score under the parameters BEFORE
 *      this window's update.  Every other element of out_logprob is 0.
 *   4. The update, g = the gradient of that pass, c = clip_norm > 0 ? clip_norm / max(gnorm, clip_norm) : 1 with gnorm by the handle's
 *      norm convention (fsmg_config.clip_norm_mode), derived as the MAML inner step derives it:
 *        FSMG_DYNEVAL_SGD: theta_l <- theta_l - lr c g + decay (theta_g - theta_l)
 *        FSMG_DYNEVAL_RMS: theta_l <- theta_l - lr c g / (sqrt(MS) + eps) + decay (theta_g - theta_l) min(1 / decay, sqrt(MS) / mean_rms)
 *      MS = ms_sum / count per parameter (the statistics below); mean_rms = the mean of sqrt(MS) over the logical elements of the
 *      fsmg_num_params tensors (pad elements of the flat buffer are not counted).  decay == 0: the last term is absent.
 *      adapt_reported == 0: a reported block is scored with ONE window [0, T) and no update.
 *   5. Pads stay exact zeros (g, theta_g and ms_sum are 0 there; eps > 0 is required for RMS).
 * On return, whatever happened: theta is back, bitwise; the Adam slots and global_step are untouched; no gradient is pending
 * (fsmg_apply_update returns FSMG_ERR_STATE); a handle with a communicator has made no collective call.
 * out_row_nll [n_rows]: for a reported row minus the fp64 sum of the row's out_logprob in position order, rounded once, computed on
 * the host from the returned array (0 for a row that only adapts); out_nll = minus the fp64 sum of every reported row's out_logprob in (row, position) order, divided by
 * the count of scored positions, rounded once (NaN when nothing is reported).  out_logprob [n_rows][T] holds zeros in the rows that
 * only adapt.  Any output pointer may be NULL.
 * A persistent kernel's time-out anywhere puts theta back and repeats the whole call once on per-step launches, as fsmg_maml_eval does.
 *
 * DELIBERATE DIFFERENCE from the paper, which carries the hidden state across segments and truncates BPTT at the segment start: here
 * every window's pass recomputes the prefix [0, lo) at the current theta_l from the zero state and differentiates through it.  The
 * library's passes start from the zero state, songs are at most max_len positions, and this variant is exactly differentiable (it has
 * a plain fp64 restatement: tests/dyneval_ref.py).  Its cost is ceil(T / S) full passes per block.  A carried initial state is not
 * offered.
 *
 * Statistics: ms_sum (one float per parameter element, fsmg_get_param's layout) and count.  fsmg_dyneval_stats_accumulate adds g * g
 * (fp32: ms_sum <- ms_sum + g * g, two roundings) of the gradient the last fsmg_forward_backward* call left and increments count;
 * FSMG_ERR_STATE without a pending gradient or when that pass was skipped on the device.  _reset zeroes both.  _get / _set move one
 * tensor's ms_sum (count = rows * cols; _set refuses a negative or non-finite value), _set_count sets count (>= 0), _info returns
 * count and mean_rms (0 while count == 0), recomputed on the device in a fixed order whenever the statistics have changed.
 *
 * fsmg_dyneval_eval_step: per artist n of the episode (support [N][K][T], query [N][Q][T], lengths [N][K] / [N][Q], either may be
 * NULL) a fresh theta_l and the stream (support rows of n, then query rows of n) with first_reported = K; *nll = minus the fp64 sum of
 * all artists' reported log-probs in (artist, row, position) order over the count of scored query positions, rounded once.
 * fsmg_dyneval_generate: adapts on the support stream (n_support_rows rows, nothing reported), runs what fsmg_generate_filtered runs at
 * theta_l (filters may be NULL), then restores theta.
 *
 * Errors, all before any device work and with nothing touched: FSMG_ERR_INVALID for a NULL handle / config / tokens, struct_size not
 * sizeof(fsmg_dyneval_config), nonzero reserved, rule not SGD / RMS, seg_len outside [1, T], rows_per_step outside [1, 2^20] (a pass's
 * capacity; the activation scratch grows on demand), lr negative or not finite, decay outside [0, 1], eps not > 0 or not finite (RMS),
 * clip_norm negative or not finite, adapt_reported not 0 / 1, n_rows outside [1, 2^20], first_reported outside [0, n_rows], a length
 * outside [1, T], K < 1 or Q < 1 (eval_step), what fsmg_generate_filtered refuses (generate); FSMG_ERR_TOKEN_RANGE for a token outside
 * [0, input_size); FSMG_ERR_STATE for RMS with count == 0.  Host tokens and lengths only. */
enum { FSMG_DYNEVAL_SGD = 0, FSMG_DYNEVAL_RMS = 1 };
typedef struct {
    int32_t struct_size;      /* sizeof(fsmg_dyneval_config), else FSMG_ERR_INVALID  */
    int32_t rule;             /* FSMG_DYNEVAL_SGD / FSMG_DYNEVAL_RMS                  */
    int32_t seg_len;          /* S in [1, T]                                          */
    int32_t rows_per_step;    /* rows per block, >= 1                                 */
    float lr;
    float decay;              /* in [0, 1]                                            */
    float eps;                /* > 0 for RMS                                          */
    float clip_norm;          /* 0: no clipping                                       */
    int32_t adapt_reported;   /* 1: adapt on the reported rows too (after scoring)    */
    int32_t reserved;         /* 0                                                    */
} fsmg_dyneval_config;
int fsmg_dyneval_stats_reset(fsmg_handle h);
int fsmg_dyneval_stats_accumulate(fsmg_handle h);
int fsmg_dyneval_stats_info(fsmg_handle h, int64_t* count, float* mean_rms);
int fsmg_dyneval_stats_get(fsmg_handle h, const char* name, float* sum, int64_t n);
int fsmg_dyneval_stats_set(fsmg_handle h, const char* name, const float* sum, int64_t n);
int fsmg_dyneval_stats_set_count(fsmg_handle h, int64_t count);
int fsmg_dyneval_score(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* tokens, const int32_t* lengths, int32_t n_rows,
                       int32_t first_reported, float* out_logprob, float* out_row_nll, float* out_nll);
int fsmg_dyneval_eval_step(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* support, const int32_t* query,
                           const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* nll);
int fsmg_dyneval_generate(fsmg_handle h, const fsmg_dyneval_config* cfg, const int32_t* support, const int32_t* support_len,
                          int32_t n_support_rows, const fsmg_gen_config* gen_config, const fsmg_gen_filters* filters,
                          const int32_t* primer, int32_t* out_tokens, float* out_logprob);

/* ---- Meta-SGD: learned per-parameter inner rates for the MAML-style step (Li et al. 2017, first order).
 * The MAML-style step learns the initialisation theta; its fine-tuning procedure is one hand-set scalar inner_lr on a clipped SGD
 * step.  With Meta-SGD enabled the handle also holds a rate per parameter element, A, a MULTIPLIER of the call's inner_lr, trained
 * with theta by the outer update.  While enabled, EVERY adaptation in the library takes step 1 below in place of the plain inner
 * step: the train, eval, masked and indexed forms of fsmg_maml_*, and fsmg_maml_generate* / fsmg_maml_beam_search* / fsmg_maml_score*.
 * No existing signature changes; disabled (or never enabled), every path is bit for bit what it was.
 *
 * State, created by the first fsmg_msgd_enable and kept until fsmg_destroy, five buffers laid out like the flat parameter buffer
 * (fsmg_get_param's layout by name; not counted by fsmg_state_bytes): A the rates, AM / AV their Adam slots, S the sum of the applied
 * support gradients of the last train-form adaptation, GA the gradient with respect to A.  Pad elements of A never matter (g is an
 * exact 0 there, so the pads of theta' stay 0 whatever A holds); the pads of S and GA are zeros.
 *
 *   1. Inner step i.  The pass, the norm, the conditions under which the step is skipped and the fp32 scalar
 *      step = (float)(clip / max(gnorm, clip)) * inner_lr are those of the plain inner step.  Per element j:
 *        st = step * A[j]                      (one rounding)
 *        p[j] <- p[j] - st * g[j]              (the plain step's expression with st for step: A == 1 gives the plain step's bits)
 *        S[j] <- fma(step, g[j], S[j])         (the train forms only: fsmg_maml_forward_backward* / fsmg_maml_step*)
 *      S is zeroed when the adaptation of a train form begins (a pass repeated after a time-out starts from zero again).  The eval
 *      and decoding forms neither read nor write S.
 *   2. Rate gradient.  After the query pass of a train form, GA[j] = -(G[j] * S[j]), one rounding: the first-order gradient of
 *      L_query(theta') with respect to A, the support gradients and their clip scales taken as constants.  For inner_steps == 1 it is
 *      the exact gradient.  It is pending until the next fsmg_apply_update or backward pass.
 *   3. Outer update, in fsmg_apply_update while a rate gradient is pending.  theta's clip + Adam runs exactly as without Meta-SGD.
 *      The rates: gnorm_a = sqrt(sum GA^2) * grad_scale, a plain global norm whatever clip_norm_mode;
 *      scale = alpha_clip_norm > 0 ? alpha_clip_norm / max(gnorm_a, alpha_clip_norm) * grad_scale : grad_scale; the step size is
 *      theta's schedule (exponential decay, Adam bias correction) with alpha_lr in place of lr at the same global_step; the element
 *      update is theta's Adam element, then A <- min(max(A, alpha_min), alpha_max).  A step that is skipped for theta (a time-out, a
 *      token out of range) is skipped for A, AM and AV too; global_step counts once.  alpha_lr == 0: A, AM and AV stay bitwise.
 *   4. Data-parallel.  GA is formed per rank BEFORE any exchange (a product of means is not a mean of products): all-reduce the
 *      buffer of fsmg_msgd_grad_buffer next to fsmg_grad_buffer, then fsmg_apply_update(1 / world).  The library's own exchange does
 *      not carry GA: fsmg_msgd_enable on a handle with a communicator, and fsmg_comm_init / _attach on an enabled handle, return
 *      FSMG_ERR_STATE.
 *
 * fsmg_msgd_enable: the first call allocates and sets A = alpha_init, AM = AV = 0; a later call keeps the state and takes the new
 * scalars (alpha_init is then unused).  fsmg_msgd_disable: every path is the old one; the state is kept.  fsmg_msgd_info: out =
 * {enabled, allocated, elements per buffer (the flat count, pads included), rate gradient pending}.  fsmg_msgd_fill: A = value, AM =
 * AV = 0.  _get_alpha / _set_alpha, _get_opt_state / _set_opt_state, _get_grad move one tensor by name (count = rows * cols);
 * _get_grad returns FSMG_ERR_STATE without a pending rate gradient.  fsmg_debug_read("msgd_sum:<name>") reads S.
 * Errors, before any device work: FSMG_ERR_INVALID for a NULL handle / config, struct_size not sizeof(fsmg_msgd_config), nonzero
 * reserved, a NaN anywhere, alpha_init not finite, alpha_lr or alpha_clip_norm negative or not finite, alpha_min > alpha_max (an
 * infinite alpha_min / alpha_max is an open end of the clamp), a non-finite value given to _fill / _set_alpha; FSMG_ERR_STATE for the calls that need the state before the
 * first fsmg_msgd_enable. */
typedef struct {
    int32_t struct_size;      /* sizeof(fsmg_msgd_config), else FSMG_ERR_INVALID     */
    float alpha_init;         /* A of the first enable                               */
    float alpha_lr;           /* >= 0; 0: the rates are not trained                  */
    float alpha_min;          /* clamp after every update of A                       */
    float alpha_max;
    float alpha_clip_norm;    /* 0: no clipping of GA                                */
    int32_t reserved;         /* 0                                                   */
} fsmg_msgd_config;
int fsmg_msgd_enable(fsmg_handle h, const fsmg_msgd_config* cfg);
int fsmg_msgd_disable(fsmg_handle h);
int fsmg_msgd_info(fsmg_handle h, int64_t out[4]);
int fsmg_msgd_fill(fsmg_handle h, float value);
int fsmg_msgd_get_alpha(fsmg_handle h, const char* name, float* host, int64_t count);
int fsmg_msgd_set_alpha(fsmg_handle h, const char* name, const float* host, int64_t count);
int fsmg_msgd_get_opt_state(fsmg_handle h, const char* name, float* m, float* v, int64_t count);
int fsmg_msgd_set_opt_state(fsmg_handle h, const char* name, const float* m, const float* v, int64_t count);
int fsmg_msgd_get_grad(fsmg_handle h, const char* name, float* host, int64_t count);
int fsmg_msgd_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count);

/* ---- Learned optimiser: a meta-learner LSTM for the MAML-style step (Ravi & Larochelle 2017, first order).
 * Meta-SGD learns one fixed rate per element; this learns a RULE: a forget gate and an input gate per parameter element, computed from
 * that element's support gradient, the support loss, the element's value and the previous gates, with fourteen weights Phi shared by
 * all elements and trained with theta by the outer update.  While enabled, EVERY adaptation in the library takes step 1 below in place
 * of the plain inner step (the forms Meta-SGD lists).  First order like the step it extends: the support gradients g_t, the support
 * losses L_t and the clip scales are constants of the meta-gradient (the paper's own assumption).  No existing signature changes;
 * never enabled, or disabled, every path is bit for bit what it was.  Meta-SGD and the learned optimiser exclude each other.
 *
 * State, created by the first fsmg_lopt_enable and kept until fsmg_destroy (not counted by fsmg_state_bytes): Phi = {wF[6], bF, wI[6],
 * bI}, its Adam slots and gradient GPhi[14]; two buffers F, I laid out like the flat parameter buffer (the gates of the previous inner
 * step); a store of max_train_steps flat support gradients with the scalars step_t, L_t per step; reduction partials.
 *
 *   1. Inner step t (1-based), element j.  The pass, the norm, the conditions under which the step is skipped and the fp32 scalar
 *      step_t = (float)(clip / max(gnorm, clip)) * inner_lr are those of the plain inner step; L_t is the support loss of the pass.
 *        prep(x) = (log|x| / 10, sign x)  where |x| >= e^-10,   (-1, e^10 x)  otherwise
 *        (a1, a2) = prep(g_t[j]);  (c1, c2) = prep(L_t)
 *        xF = (a1, a2, c1, c2, theta_{t-1}[j], F_{t-1}[j]);  xI = (a1, a2, c1, c2, theta_{t-1}[j], I_{t-1}[j]);  F_0 = 1, I_0 = 0
 *        f = sigmoid(wF . xF + bF);  i = sigmoid(wI . xI + bI)       (the dot product: fma by fma from the bias, in the order of x)
 *        q = f * theta_{t-1}[j]                                      (one rounding, never contracted)
 *        st = step_t * (gate_scale * i)                              (two roundings)
 *        theta_t[j] = q - st * g_t[j]                                (the plain step's expression with q for p and st for step)
 *      F, I restart from F_0, I_0 whenever an adaptation begins (a repeat after a time-out is a beginning).  With w = 0, bF large
 *      (f == 1), bI = 0 and gate_scale = 2 the step is the plain step bit for bit.  The train forms (fsmg_maml_forward_backward*,
 *      fsmg_maml_step*, fsmg_maml_tasks_forward_backward / _step) also store g_t, step_t, L_t and refuse inner_steps >
 *      max_train_steps (FSMG_ERR_INVALID) before any pass; eval, scoring and decoding forms store nothing and take up to 64 steps.
 *   2. Meta-gradient, behind the query pass of a train form (per-artist forms: behind each artist's query pass, before the fold).
 *      Per element D = G[j], carryF = carryI = 0; for t = K .. 1:
 *        dF = D theta_{t-1} + carryF;  dI = -D step_t gate_scale g_t + carryI;  pf = dF f(1 - f);  pi = dI i(1 - i)
 *        GwF += pf xF;  GbF += pf;  GwI += pi xI;  GbI += pi
 *        D <- D f + pf wF[4] + pi wI[4];  carryF = pf wF[5];  carryI = pi wI[5]
 *      then G[j] <- D: the outer gradient of theta is the gradient through the learned rule.  GPhi is the sum over elements in fp64
 *      (pads contribute an exact 0), rounded to fp32 once; the per-artist forms fold the artists' sums with weight 1 / N in fixed
 *      order in fp64.  inner_steps == 0: G stays, GPhi = 0.  Pending until the next fsmg_apply_update or backward pass.
 *   3. Outer update, in fsmg_apply_update while a GPhi is pending and phi_lr > 0.  theta's clip + Adam runs unchanged on the rewritten
 *      G.  Phi: gnorm = sqrt(sum GPhi^2) * grad_scale; scale = phi_clip_norm > 0 ? phi_clip_norm / max(gnorm, phi_clip_norm) *
 *      grad_scale : grad_scale; theta's schedule with phi_lr in place of lr at the same global_step; theta's Adam element.  Skipped
 *      wherever theta's step is skipped.  phi_lr == 0: Phi and its slots stay bitwise.
 *   4. Data-parallel.  GPhi is formed per rank BEFORE any exchange: all-reduce the 14 floats of fsmg_lopt_grad_buffer beside
 *      fsmg_grad_buffer, then fsmg_apply_update(1 / world).  A handle with a library communicator refuses fsmg_lopt_enable, and an
 *      enabled handle refuses fsmg_comm_init / _attach (FSMG_ERR_STATE).
 *
 * fsmg_lopt_enable: the first call allocates and sets w = 0, bF = bF_init, bI = bI_init, slots 0; a later call keeps Phi and the
 * slots and takes the new scalars (the store grows where max_train_steps did); captured graphs are dropped.  fsmg_lopt_disable: every
 * path is the old one; the state is kept.  fsmg_lopt_info: out = {enabled, allocated, max_train_steps, GPhi pending}.  _get_phi /
 * _set_phi / _get_grad move 14 floats, _get_opt_state / _set_opt_state 14 + 14; _get_grad returns FSMG_ERR_STATE without a pending
 * GPhi.  fsmg_debug_read: "lopt_F:<name>", "lopt_I:<name>" the gates after the last inner step, "lopt_g<t>:<name>" the stored g_t
 * (t from 0), "lopt_scalars" {step_t[8], L_t[8]}, "lopt_theta:<name>" the theta_K the back-propagation replayed (written only while
 * keep_adapted is set).
 * Errors, before any device work: FSMG_ERR_INVALID for a NULL handle / config, struct_size not sizeof(fsmg_lopt_config), nonzero
 * reserved, a NaN or non-finite value anywhere, phi_lr or phi_clip_norm negative, gate_scale <= 0, max_train_steps outside [1, 8], a
 * non-finite value given to _set_phi / _set_opt_state; FSMG_ERR_STATE with Meta-SGD enabled (and fsmg_msgd_enable with the learned
 * optimiser enabled), with a communicator, and for the calls that need the state before the first fsmg_lopt_enable. */
typedef struct {
    int32_t struct_size;      /* sizeof(fsmg_lopt_config), else FSMG_ERR_INVALID            */
    float bF_init;            /* bF of the first enable (6: f = 0.9975)                     */
    float bI_init;            /* bI of the first enable (0: i = 1/2)                        */
    float gate_scale;         /* > 0; 2: bI = 0 is the plain rate                           */
    float phi_lr;             /* >= 0; 0: Phi is not trained                                */
    float phi_clip_norm;      /* 0: no clipping of GPhi                                     */
    int32_t max_train_steps;  /* 1 .. 8: inner steps a train form may take (and store)      */
    int32_t reserved;         /* 0                                                          */
} fsmg_lopt_config;
#define FSMG_LOPT_NPHI 14
int fsmg_lopt_enable(fsmg_handle h, const fsmg_lopt_config* cfg);
int fsmg_lopt_disable(fsmg_handle h);
int fsmg_lopt_info(fsmg_handle h, int64_t out[4]);
int fsmg_lopt_get_phi(fsmg_handle h, float phi[FSMG_LOPT_NPHI]);
int fsmg_lopt_set_phi(fsmg_handle h, const float phi[FSMG_LOPT_NPHI]);
int fsmg_lopt_get_opt_state(fsmg_handle h, float m[FSMG_LOPT_NPHI], float v[FSMG_LOPT_NPHI]);
int fsmg_lopt_set_opt_state(fsmg_handle h, const float m[FSMG_LOPT_NPHI], const float v[FSMG_LOPT_NPHI]);
int fsmg_lopt_get_grad(fsmg_handle h, float gphi[FSMG_LOPT_NPHI]);
int fsmg_lopt_grad_buffer(fsmg_handle h, void** device_ptr, int64_t* count);

/* ---- Dropout for the train passes (Zaremba et al. 2014: non-recurrent connections only).  Never enabled, or
 * disabled, every path is what it was, bit for bit.  The masks are never stored: forward and backward regenerate them from a
 * counter-based generator (Philox4x32-10, Salmon et al. 2011), so a test can rebuild every mask on the host.
 *
 * Sites.  Site 0 is the embedding rows that enter layer 0 (width embedding_size).  Site l + 1 is the output h^l_t of layer l on its
 * way UP (width hidden_size): for l < n_layers - 1 to layer l + 1's input product, for the top layer to the projection.  The
 * recurrent path h^l_t -> h^l_{t+1} and the cell state are never masked.  Site 0 uses keep_input, every other site keep_output.
 * A site whose keep is exactly 1 launches nothing and is bit-identical to the undropped path.
 *
 * Mask of element (row, j) at `site` in pass p: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (j >> 2, row, site, p mod 2^32); element j takes output word j & 3.  row = t * B + b, the device's time-major row order of the
 * pass (B = its sequences, support rows first); with variational = 1, row = b: one mask per song shared by all time steps (Gal &
 * Ghahramani 2016).  The element is kept iff (word >> 8) < thr, thr = (uint32)(keep * 16777216.0f) (truncation).  Kept elements
 * are multiplied by scale = 1.0f / keep (one fp32 rounding of the quotient, one of the product), dropped elements are +0.0, pad
 * columns stay zero.  Backward: the gradient that flows back through a site is multiplied by the same mask * scale, regenerated.
 *
 * Which passes.  Dropout is on in the gradient passes of the train forms: fsmg_train_step*, fsmg_forward_backward*, and
 * fsmg_maml_step* / fsmg_maml_forward_backward* (the inner support passes and the query pass).  It is never on in fsmg_eval_*,
 * fsmg_score*, any decoding, fsmg_cache_*, fsmg_dyneval_*, nor in the adaptation passes of fsmg_maml_eval* and the MAML decode /
 * score entry points.
 *
 * Pass index.  A 64-bit counter of the handle gives every dropped gradient pass its own p (a MAML-style step uses inner_steps + 1
 * of them); a pass repeated inside one call after a time-out draws the masks of the pass it repeats.  fsmg_dropout_info: out =
 * {enabled, index of the last dropped pass (-1: none yet), index the next one takes, bytes of the masked copies}.
 * fsmg_dropout_set_pass sets the next index (checkpoint restore, tests).
 *
 * Order.  A dropped pass runs in the serial, single-stream, eager order (the XCD-partitioned order's gated projection would read
 * the top layer's rows before a masked copy of them can exist); inside it every kernel choice stays the handle's.  A handle that
 * is enabled with both keeps 1 takes that order too and launches nothing else.
 *
 * fsmg_dropout_enable takes the scalars (a later call replaces them; the pass counter is kept) and allocates the masked copies
 * ([T * B][Ep] + n_layers x [T * B][Hp] floats, outside fsmg_state_bytes, freed by fsmg_destroy).  fsmg_dropout_mask writes the
 * 0 / 1 bytes [T * B][width] (device row order) of `site` in pass `pass` for B sequences with the enabled scalars, keep 1 included.
 * fsmg_debug_read("drop<site>") returns the masked activations [T * B][Ep or Hp] of the last dropped pass.
 * Errors, before any device work: FSMG_ERR_INVALID for a NULL handle / config / out, struct_size not
 * sizeof(fsmg_dropout_config), a keep outside (0, 1] or NaN, variational not 0 / 1, pass < 0, a site outside [0, n_layers], B < 1;
 * FSMG_ERR_STATE for fsmg_dropout_mask / _set_pass before the first fsmg_dropout_enable and for "drop<site>" without a dropped
 * pass at that site. */
typedef struct {
    int32_t struct_size;      /* sizeof(fsmg_dropout_config), else FSMG_ERR_INVALID  */
    float keep_input;         /* site 0, in (0, 1]                                   */
    float keep_output;        /* sites 1 .. n_layers, in (0, 1]                      */
    int32_t variational;      /* 1: one mask per song, shared by all time steps      */
    uint64_t seed;
} fsmg_dropout_config;
int fsmg_dropout_enable(fsmg_handle h, const fsmg_dropout_config* cfg);
int fsmg_dropout_disable(fsmg_handle h);
int fsmg_dropout_info(fsmg_handle h, int64_t out[4]);
int fsmg_dropout_set_pass(fsmg_handle h, int64_t next_pass);
int fsmg_dropout_mask(fsmg_handle h, int64_t pass, int32_t site, int32_t B, uint8_t* out);

/* ---- batched passes from a carried LSTM state: truncated BPTT, scoring and evaluation over segments.
 * Every batched pass above starts each row from a zero state and reads [start word, x_0 .. x_{T-2}].  A STATE PASS starts from a decode
 * state (fsmg_dstate_*, above) and leaves it advanced, on the train path's kernels: one persistent launch per layer and direction and
 * one projection GEMM per pass, where fsmg_dstate_feed pays a launch per position and layer.  A song longer than max_len is walked in
 * segments of T = max_len tokens on one state: scored or evaluated under its full context, trained with truncated BPTT.
 * A state pass over tokens [R][T] (R == the state's rows, ids in [0, input_size); host, or device with c->tokens_on_device) takes
 * optional HOST lengths [R], each in [0, T], NULL = all T, at least one > 0 (host memory even with device tokens: the host must know them).
 *   Inputs     row b reads [pending_b, x_0 .. x_{T-2}], pending_b the state's pending token (the start word on a fresh state), against
 *              the targets x_0 .. x_{T-1}.  Layer l starts from the state's h[l][b], c[l][b] instead of zeros.
 *   Scored     position t iff t < len[b].  Weights, n_valid, loss and dlogits are those of the masked passes with one
 *              group over all R rows; positions t >= len[b] get the masked passes' fixed ids (input: the start word, target: 0), so
 *              nothing depends on what the caller put behind a row's end.  A row with len[b] == 0 reads the start word at position 0 too.
 *   Gradients  those of the segment with the incoming state held CONSTANT (truncated BPTT): nothing flows into the previous segment --
 *              dh, dc arriving at slot 0 are dropped -- and the recurrent weight gradient includes h_{-1}^T dZ_0 with the imported h.
 *              The embedding gradient of position 0 goes to the pending token's row.
 *   State      after a successful call h[l][b], c[l][b] are slot len[b] of the pass's hidden / cell states, bit for bit (len[b] == T: the
 *              end of the segment; len[b] == 0: the row's state as it was).  The context gains the T tokens y[b][t] = x[b][t] for
 *              t < len[b] and, behind them, the last real token repeated (x[b][len[b]-1], or the old pending token when len[b] == 0): the
 *              rows stay in lockstep, n_ctx += T, n_gen is unchanged, the last context token -- x[b][len[b]-1] -- is pending.  The
 *              repetition penalty counts distinct ids, so the repeats add nothing to its set.
 *   Untouched  an argument error, a token-range error and a skipped step leave the state exactly as it was (host tokens are checked
 *              before any device work; device tokens and time-outs by the flag the pass raises on the device: the export reads it).
 *   Time-out   a persistent kernel's time-out repeats the pass on per-step launches as everywhere else; the repeat imports the same
 *              state again and the state advances once.
 *   Order      a state pass runs the serial order -- single-stream, eager, no XCD-partitioned or two-stream order, no graph replay --
 *              and inside it every kernel choice (recurrence family, GEMM kernels, fused softmax) is the handle's.  Enabled dropout
 *              composes (non-recurrent sites only); a dropped state pass takes a pass index like any dropped train pass.
 * On a fresh state every call is bitwise its masked twin over one pass of R rows (fsmg_score_masked, fsmg_eval_step_masked,
 * fsmg_forward_backward_masked, fsmg_train_step_masked with N = 1, K = 0, Q = R).  Every stateless entry point returns the bits it
 * returned before state passes existed.
 *   fsmg_score_state             fsmg_score's five outputs ([R][T], out_row_nll [R]; any may be NULL, not all) treated as fsmg_score_masked
 *                                treats them: 0 behind a row's end, out_row_nll over the scored positions (NaN for a row of length 0).
 *                                Advances st; changes nothing else that fsmg_score does not change.
 *   fsmg_eval_step_state         *nll = the segment's summed NLL over its n_valid (fsmg_eval_step_masked's number for one group);
 *                                *n_valid (may be NULL) = the sum of the lengths, so that segments combine as sum(nll_i n_i) / sum(n_i).
 *                                Advances st.
 *   fsmg_forward_backward_state  loss and gradients as above, then fsmg_apply_update -- fsmg_forward_backward_masked's contract (loss
 *                                ring, buckets, fsmg/dist.py's forward/backward + all-reduce + apply route).  Advances st; synchronises
 *                                the stream once to learn whether the device advanced it.
 *   fsmg_train_step_state        the fused step, fsmg_train_step_masked's contract with a non-NULL loss (the read-back is how the call
 *                                learns that the step and the state went through; a timed-out step is repeated inside).  Advances st.
 * MAML-style, Meta-SGD, cache and dynamic-evaluation calls stay stateless.
 * Errors, before any device work and with nothing touched: FSMG_ERR_INVALID for a state this handle does not own, more rows than
 * FSMG_STATE_PASS_ROWS, a length outside [0, T] or all lengths 0, a wrong version or nonzero reserved fields, tokens_on_device not
 * 0 / 1, NULL tokens (or config, or the outputs named above); FSMG_ERR_TOKEN_RANGE for a host id outside [0, input_size);
 * FSMG_ERR_STATE for the two gradient calls on a handle with a library communicator (fsmg_comm_*): a step that a peer rank makes every
 * rank skip would leave this rank's state advanced -- exchange the gradients outside the library (fsmg/dist.py). */
#define FSMG_STATE_CONFIG_VERSION 1
#define FSMG_STATE_PASS_ROWS 1024          /* rows of one state pass at the most */
typedef struct fsmg_state_config {
    int32_t version;            /* FSMG_STATE_CONFIG_VERSION                                   */
    int32_t tokens_on_device;   /* 0 / 1                                                       */
    int32_t reserved[6];        /* must be 0                                                   */
} fsmg_state_config;
int fsmg_score_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths,
                     float* out_logprob, int32_t* out_rank, float* out_entropy, int32_t* out_argmax, float* out_row_nll);
int fsmg_eval_step_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths,
                         float* nll, int32_t* n_valid);
int fsmg_forward_backward_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths);
int fsmg_train_step_state(fsmg_handle h, fsmg_dstate st, const fsmg_state_config* c, const int32_t* tokens, const int32_t* lengths,
                          float* loss);

/* ---- per-artist MAML: one adaptation per artist.  fsmg_maml_forward_backward adapts once, on the N * K support rows of
 * all N artists, and takes the query gradient of all N * Q rows at that one theta'.  The calls below treat the episode as a meta-batch of
 * N tasks: support [N][K][max_len], query [N][Q][max_len], optional lengths [N][K] / [N][Q].  For artist n = 0 .. N-1 in that order,
 * w = (float)(1.0 / N):
 *   1. adapt: theta' starts at theta and takes inner_steps inner steps on artist n's K support rows alone -- exactly the adaptation of
 *      fsmg_maml_forward_backward (or _masked, with lengths) for N = 1, K: the pass, the norm of that artist's gradient, the clip, the
 *      skip conditions, the Meta-SGD element step and its S (zeroed per artist), dropout's pass counter.
 *   2. query pass: the K = 0 train pass over artist n's Q query rows at theta'_n: G_n, its tail, the loss L_n (masked: over artist n's
 *      own n_valid -- a mean of per-artist means, the convention of the episode-parallel exchange).
 *   3. fold, one launch: n == 0: ACC[j] = w * G_n[j], one rounding (N == 1: nothing is folded, G keeps its bits, -0 included);
 *      n > 0: ACC[j] = fma(w, G_n[j], ACC[j]); the last artist's result goes to the flat gradient buffer, so fsmg_grad_buffer, the
 *      buckets and fsmg_get_grad see the folded gradient.  Tail: [0] folds with w * w (the N IndexedSlices concatenated), [1] with w,
 *      [2] .. [5] are non-zero if any artist's was.  Meta-SGD enabled: GA_n[j] = -(G_n[j] * S_n[j]), one rounding, folded by the same
 *      rule into the rate gradient.  Theta comes back in the same launch; pad elements stay exact zeros.
 *   4. afterwards theta is back bitwise whatever happened, Adam slots and global_step are untouched, a gradient (and with Meta-SGD a rate
 *      gradient) is pending for fsmg_apply_update(grad_scale); fsmg_debug_set("keep_adapted", 1) keeps theta' of artist N - 1.
 * N == 1: every tasks call has the bits of its fsmg_maml_* twin.  Any N: theta'_n, G_n and L_n have the bits of N separate N = 1 calls of
 * the existing entry points on the same handle state; the returned buffer is their fold by the rule above.
 * fsmg_maml_tasks_eval: per artist the eval-form adaptation (never dropped, S untouched) and the query NLL_n of fsmg_maml_eval / _masked
 * for N = 1; *nll = (float)(sum_n (double)NLL_n / N), in artist order.  No gradient is pending afterwards.
 * support_len == query_len == NULL selects the unmasked passes; one NULL and one non-NULL is FSMG_ERR_INVALID.  table_id >= 0: support /
 * query are host row indices into that table, support_len / query_len must be NULL and use_table_lengths says whether the pass is masked.
 * fsmg_maml_tasks_step is to fsmg_maml_tasks_forward_backward what fsmg_maml_step is to fsmg_maml_forward_backward: loss == NULL leaves
 * the loss in the ring, an attached communicator makes it the library-owned exchange, and after a time-out the whole call is repeated
 * once on per-step launches with dropout's pass counter put back.  task_loss / task_nll [N] are read back only when non-NULL;
 * fsmg_debug_read("task_loss") reads the [N] losses L_n of the last tasks train call.  Timing classes "task_fold" (the fold's kernel)
 * and "tasks" (a train call's loop over the artists).
 * Errors, before any device work and with nothing touched: FSMG_ERR_INVALID for a NULL handle / config / token pointer, struct_size not
 * sizeof(fsmg_maml_tasks_config), nonzero reserved words, inner_steps outside [0, 64], inner_lr negative or NaN, tokens_on_device or
 * use_table_lengths not 0 / 1, table_id outside [-1, 4), use_table_lengths or a length pointer at odds with table_id, a bad N / K / Q,
 * a host length outside [1, max_len].  FSMG_ERR_STATE for a table (or its lengths) that was never uploaded.  A token or length out of
 * range in any artist skips the update on the device and returns FSMG_ERR_TOKEN_RANGE. */
typedef struct {
    int32_t struct_size;       /* sizeof(fsmg_maml_tasks_config), else FSMG_ERR_INVALID          */
    int32_t inner_steps;       /* [0, 64]                                                        */
    float   inner_lr;          /* >= 0                                                           */
    int32_t tokens_on_device;  /* 0 / 1; covers tokens and lengths                               */
    int32_t table_id;          /* -1: tokens; [0, 4): host row indices into that table           */
    int32_t use_table_lengths; /* 0 / 1, only with table_id >= 0                                 */
    int32_t reserved[2];       /* must be 0                                                      */
} fsmg_maml_tasks_config;
int fsmg_maml_tasks_forward_backward(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                                     const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q);
int fsmg_maml_tasks_step(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                         const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* loss, float* task_loss);
int fsmg_maml_tasks_eval(fsmg_handle h, const fsmg_maml_tasks_config* c, const int32_t* support, const int32_t* query,
                         const int32_t* support_len, const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float* nll, float* task_nll);

/* ---- unigram baseline.  Replaces the graph of UnigramModel (src/models/unigram_model.py:26-39): a
 * word_count variable initialised to alpha = 1, tf.scatter_add of ones, prob = gather(word_count) / reduce_sum(word_count),
 * loss = -mean(log prob).  Counts live on the device as unsigned integers (exact, order-independent atomics) and cross the
 * boundary as float32 like the reference's variable.  `words` is a flat int32 array (host, or device when on_device != 0) of ids
 * in [0, input_size); an id outside -> FSMG_ERR_TOKEN_RANGE (counts untouched by that call's NLL, the update skips the id). */
typedef struct fsmg_unigram* fsmg_unigram_handle;
int fsmg_unigram_create(int32_t input_size, int32_t device, fsmg_unigram_handle* out);
int fsmg_unigram_destroy(fsmg_unigram_handle u);
const char* fsmg_unigram_last_error(fsmg_unigram_handle u);     /* NULL: the text of a failed fsmg_unigram_create */
/* *nll = -mean(log(count[w] / sum(counts))) over the n words, counts as they are (unigram_model.py:35-37) */
int fsmg_unigram_nll(fsmg_unigram_handle u, const int32_t* words, int64_t n, int32_t on_device, float* nll);
/* counts[w] += 1 per word (unigram_model.py:31-33); with loss != NULL the NLL of the same words BEFORE the update is returned
 * (UnigramModel.train fetches both in one sess.run) */
int fsmg_unigram_train(fsmg_unigram_handle u, const int32_t* words, int64_t n, int32_t on_device, float* loss);
int fsmg_unigram_get_counts(fsmg_unigram_handle u, float* host, int64_t count);
int fsmg_unigram_set_counts(fsmg_unigram_handle u, const float* host, int64_t count);
/* argmax of the counts, lowest id on ties (UnigramModel.sample, unigram_model.py:71-78) */
int fsmg_unigram_argmax(fsmg_unigram_handle u, int32_t* word);

/* last n train losses (oldest first), n <= 1024; synchronises the stream */
int fsmg_read_losses(fsmg_handle h, float* out, int32_t n);

/* What the handle has been doing (synchronises the stream).  A train step whose persistent recurrent kernel timed out
 * (its blocks were not co-resident: another workload held the CUs) or whose batch held an out-of-range token is SKIPPED
 * on the device -- parameters, Adam state, global_step untouched -- and tallied here; after a time-out the handle runs
 * `fallback` train steps with one launch per time step and then tries the persistent kernels again.  With loss != NULL
 * fsmg_train_step repeats a timed-out step itself; with loss == NULL the episode stays skipped, so a throughput loop
 * must compare fsmg_get_step / these counters with the number of steps it issued (bench.py does). */
typedef struct fsmg_stats {
    int64_t timeouts;                   /* time-outs noticed by the host (each one starts a fallback period)        */
    int64_t steps_skipped_timeout;      /* train steps the device skipped because of a time-out (own or a peer rank) */
    int64_t steps_skipped_token_range;  /* train steps the device skipped because a token id was out of range        */
    int64_t xcd_launches;               /* launches of the XCD-local persistent kernels (hidden size 512)            */
    int64_t persistent_launches;        /* launches of the column-split persistent kernels                           */
    int64_t step_launches;              /* one-launch-per-time-step recurrent launches                               */
    int32_t persistent_path;            /* 1: persistent kernels are in force right now                              */
    int32_t fallback_steps_left;
    int64_t steps_skipped_peer_failure; /* train steps every rank skipped because one rank failed before the exchange (library-owned exchange) */
    int64_t xov_selfcheck_mismatches;   /* XCD-partitioned order: 16-byte words of the gated projection's logits that differed from the
                                           same GEMM recomputed on the serial path (the self-check of a handle's first passes);
                                           non-zero = that step was skipped and repeated, the handle keeps the serial order        */
    int64_t softmax_range_rows;         /* rows outside the range of the shift-free fused softmax (sum_v exp(logit) within [e^-60, 1e30],
                                           exp(target logit) >= 1e-30): the step that held them was skipped and repeated with the
                                           cross-entropy pass, which the handle keeps from then on */
    int64_t steps_skipped_softmax_range; /* train steps the device skipped for that reason (own rows or a peer rank's: the indicator travels in
                                           the reduced gradient tail, so every rank of a data-parallel job switches in the same step) */
    int32_t aux_stream_tries;           /* second streams fsmg_create drew until one ran BESIDE the handle's own (the process's streams share a few
                                           hardware queues); -1: none did -- the XCD-partitioned / two-stream orders are off for this handle, it runs
                                           the serial order (slower, same results); fsmg_debug_set("reprobe_aux", 1) probes again */
    int32_t reserved0;
} fsmg_stats;
int fsmg_get_stats(fsmg_handle h, fsmg_stats* out);

/* ---- introspection for kernel-level parity tests and bench.py --------------------------- */
/* copy an internal activation buffer of the last forward to the host, float32:
 *   "h<l>" [T+1,B,Hp] (index 0 = zero state), "c<l>" [T+1,B,Hp], "gates<l>" [T,B,4Hp] (packed
 *   gate order, holds dz after a backward), "logits" [T*B,V1p], "lse" [T*B], "ce" [T*B];
 *   rows are TIME-major (row = t*B + b).  count = elements to copy (<= buffer size).
 *   "xcd_bx3" [1]: 1.0 when the handle runs the bf16-split XCD-local recurrent kernels (hidden 512: created for > 64 rows, or for
 *   the XCD-partitioned schedule); "aux_tries" [1]: second streams fsmg_create drew until one ran BESIDE the handle's stream (a process's
 *   streams share GPU_MAX_HW_QUEUES hardware queues; -1: none did and the handle keeps the serial order); "xcd_partitioned" [3]: 1.0 when train passes take the XCD-partitioned order, XCDs the chains occupy, whether the LAST pass took it;
 *   "gemm_kinds" [4]: GEMM launches the host has enqueued through this handle since fsmg_create, by kernel: [0] fp32 MFMA (k_gemm,
 *   k_gemm_staged, k_gemm_queue), [1] k_gemm_bx3, [2] k_gemm_bx3w (wave-specialised), [3] k_gemm_bx3h (256 x 256 tile).  A launch
 *   captured into a hipGraph counts once, when it is captured; a replay of the graph does not count again.  Which kernel a GEMM takes
 *   follows FSMG_GEMM_H / FSMG_GEMM_WS, how many K slabs FSMG_MAX_SPLIT: all three are read by fsmg_create, per handle
 *   "adapted:<parameter name>" [rows*cols]: the adapted parameters theta' of the last MAML-style call (fsmg_maml_forward_backward /
 *   _step / _eval, their _indexed and _masked forms, fsmg_maml_generate / _beam_search / _score), in the reference layout like fsmg_get_param;
 *   count must be rows*cols.  Needs fsmg_debug_set("keep_adapted", 1) before that call: FSMG_ERR_STATE if nothing has been kept */
int fsmg_debug_read(fsmg_handle h, const char* what, float* host, int64_t count);
/* run-time knobs of a handle that used to be create-time environment variables (tests, diagnostics):
 *   "chain_spin_limit"  polls before a persistent recurrent kernel gives up (0 forces the time-out path)
 *   "fallback_steps"    train steps on per-step launches after a time-out before the persistent path is tried again
 *   "persistent"        0: one launch per time step instead of the persistent recurrent kernels, 1: back (buffers permitting)
 *   "eager"             0: passes are replayed from hipGraphs wherever fsmg_config.use_graph allows, 1: passes on the persistent
 *                       recurrent kernels are issued eagerly (default)
 *   "inplace_dlogits"   1 (default): a train pass's cross entropy writes dlogits over the logits it has just read ("logits" then
 *                       reads back as dlogits after a train pass), 0: two buffers
 *   "fused_softmax"     1 (default): train passes whose projection weight gradient runs on the 256 x 256-tile kernel never materialise
 *                       dlogits: the projection stores exp(logit), one kernel per pass derives lse / loss / row scales, the two GEMMs
 *                       apply them ("logits" / "dlogits" then read back exp(logit) with the target element reduced by the row sum);
 *                       0: the cross-entropy pass
 *   "upd_split"         1: clip + Adam of an eager pass as two launches, the softmax half on the auxiliary stream beside the next
 *                       step's input phase (bit-identical; measured slower), 0 (default): one launch
 *   "upd_defer"         1 (default): under the XCD-partitioned eager order (hidden 512, one layer) the fused train step leaves the softmax
 *                       half of clip + Adam unlaunched; the next train pass runs it on the XCDs its forward chain leaves free, any other
 *                       call launches it in stream order first (bit-identical), 0: one launch.  fsmg_debug_read("upd_defer", 4)
 *                       = [knob, the half when the read began: 0 none / 1 in flight / 2 not launched, halves placed, halves launched in line]
 *                       and, alone among the reads, leaves a waiting half waiting
 *   "tail_aside"        1 (default): the bandwidth-bound tail of an eager backward pass (deferred slab sums, embedding gradient) on
 *                       the auxiliary stream beside the bottom layer's weight-gradient GEMM (bit-identical), 0: in line
 *   "xov_dk_tail"       1 (default): XCD-partitioned order, hidden 512, one layer: the merged dKx + dKh GEMM's items are the tail of the work
 *                       list that the projection weight gradient's clean-up launch drains behind the BPTT chain -- one launch instead of two
 *                       (bit-identical), 0: two launches.  2 (tests only, the pass's gradients are NOT computed): no clean-up
 *                       launch.  fsmg_debug_read("xov_dk_tail", 4) = [knob, joint launches enqueued, dW's items, dK's items of the last such
 *                       pass]; fsmg_debug_read("xov_bwd_queue", n) = the backward pair's queue words as the last pass left them ([0..1] draw
 *                       counters, [4 + i] claim word of joint item i: dW's items, then dK's)
 *   "xov_selfcheck"     XCD-partitioned order: the next `value` train passes recompute the gated projection on the serial path and
 *                       compare the words (default: the first 2 passes of a handle)
 *   "xov_selfcheck_fault" 1: the comparison runs against a buffer that is NOT the recomputed logits (tests of the recovery path)
 *   "xov_selfcheck_every" XCD-partitioned order: besides the first passes, one pass in every `value` is checked the same way for the handle's
 *                       whole life (default 1000: 0.03 % of the training time; 0: never again).  fsmg_debug_read("xov_selfcheck", 3) = [passes
 *                       checked so far, passes that took the order, the period]
 *   "reprobe_aux"       1: a handle whose create-time probe found no second stream running beside its own (fsmg_stats.aux_stream_tries = -1)
 *                       probes again (300 us, then 5 ms per candidate); on success the overlapped tails -- and the XCD-partitioned order where the
 *                       handle was created in the format it needs -- come back
 *   "keep_adapted"      1: every MAML-style call copies its adapted parameters theta' into a buffer of the handle's own (allocated on first
 *                       use, one copy kernel in stream order) right before it puts theta back; fsmg_debug_read("adapted:<name>") reads it
 *                       (tests).  0 (default): no buffer, no launch, results bit-identical either way
 * Synchronises the stream and drops the captured graphs. */
int fsmg_debug_set(fsmg_handle h, const char* what, int64_t value);
/* shader clock the chip sustains while the handle works: _begin starts a one-wave probe on a stream of its own that compares the
 * shader-clock counter with the constant 100 MHz real-time counter for `microseconds`; issue the work to be measured behind it;
 * _end waits for the probe and returns GHz (bench.py: roofline.clock_ghz -- peaks are quoted at the 2.4 GHz spec clock) */
int fsmg_debug_clock_begin(fsmg_handle h, int32_t microseconds);
int fsmg_debug_clock_end(fsmg_handle h, float* ghz);
/* padded sizes: writes Ep, Hp, V1p, last B, T */
int fsmg_debug_dims(fsmg_handle h, int32_t dims[5]);
/* diagnostics: run ONE instrumented recurrent step kernel (which = 0 forward, 1 backward) at t = T/2 on the
 * buffers of the last forward/backward (clobbers them) and return 8 s_memtime stamps per wave:
 * [0] entry, [1] operands landed, [2] partials in LDS, [3] past the block barrier, [4] done.  cap >= n_blocks*n_waves*8 */
int fsmg_debug_step_profile(fsmg_handle h, int32_t which, uint64_t* stamps, int64_t cap, int32_t* n_blocks,
                            int32_t* n_waves);
/* per-kernel-class HIP-event timing on the handle's stream (disables graph replay while on).
 * classes: "gemm_zx","lstm_fwd","gemm_logits","ce","gemm_dhout","gemm_dw","lstm_bwd",
 * "gemm_dk","gemm_dx","embed_grad","update","state_import","state_export" (the last two: state passes only) */
int fsmg_timing_enable(fsmg_handle h, int32_t on);
/* restrict event timing to ONE kernel class (NULL or "" = all classes): two event records per
 * launch of that class, cheap enough to leave on inside a throughput measurement */
int fsmg_timing_select(fsmg_handle h, const char* kernel_class);
int fsmg_timing_read(fsmg_handle h, const char* kernel_class, double* total_ms, int64_t* launches);
int fsmg_timing_reset(fsmg_handle h);

#ifdef __cplusplus
}
#endif
#endif /* FSMG_H */
