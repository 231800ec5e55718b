// Support-set neural cache: fsmg_cache_build / _create_from / _get / _info / _destroy, fsmg_cache_attend, fsmg_cache_score,
// fsmg_cache_eval_step, and their forms with per-song lengths and ragged groups (fsmg_cache_build_masked, _create_from_counts, _counts,
// _score_masked, _self_score_masked, _eval_step_masked).  Host-side C++ only (part of the C-ABI of libfsmg, include/fsmg.h); the kernels live in cache.hip (attention,
// cache fill) and score.hip (the model log-prob).  DESIGN.md 17.
#include "fsmg_model.h"

using namespace fsmg;
using namespace fsmg_host;

namespace fsmg_host {

// the cache `c` if this handle owns it (the registry: a destroyed or foreign pointer is never dereferenced)
fsmg_cache_s* find_cache(fsmg_model* h, fsmg_cache c) {
    for (fsmg_cache_s* s : h->caches)
        if (s == c && c != nullptr) return s;
    fail(h, FSMG_ERR_INVALID, "not a cache of this handle (never created here, or already destroyed)");
    return nullptr;
}

void free_cache(fsmg_cache_s* c) {
    if (c->mem) hipFree(c->mem);
    if (c->idx_mem) hipFree(c->idx_mem);
    delete c;
}

namespace {

constexpr int64_t CACHE_MAX_ENTRIES = 1LL << 22;
constexpr int64_t CACHE_MAX_KEY_BYTES = 1LL << 31;
constexpr int64_t CACHE_GEN_MAX_SCORES = 1LL << 26;     // R * Mg of one cache-conditioned call (fp64 scores: 512 MiB)
static_assert(CACHE_GEN_CHUNK == FSMG_CACHE_GEN_CHUNK, "include/fsmg.h states the key chunk of k_cache_scores");

int check_cache_size(fsmg_model* h, int64_t G, int64_t Mg) {
    if (G < 1 || Mg < 1) return fail(h, FSMG_ERR_INVALID, "a cache needs n_groups >= 1 and entries_per_group >= 1");
    if (G > CACHE_MAX_ENTRIES || Mg > CACHE_MAX_ENTRIES || G * Mg > CACHE_MAX_ENTRIES)
        return fail(h, FSMG_ERR_INVALID, "n_groups * entries_per_group must be <= 2^22");
    if (G * Mg * h->Hp * 4 > CACHE_MAX_KEY_BYTES) return fail(h, FSMG_ERR_INVALID, "the keys of a cache must fit 2^31 bytes");
    return FSMG_OK;
}

// an empty cache of G x Mg entries on the device, not yet registered; `ragged`: with the per-group counts behind the values (the
// caller fills n_g and uploads it), a uniform cache's block being what it always was
int alloc_cache(fsmg_model* h, int G, int Mg, fsmg_cache_s** out, bool ragged = false) {
    fsmg_cache_s* c = new (std::nothrow) fsmg_cache_s;
    if (!c) return fail(h, FSMG_ERR_NOMEM, "out of host memory");
    c->G = G; c->Mg = Mg; c->H = h->H; c->Hp = h->Hp;
    const size_t kbytes = (size_t)round_up((int64_t)sizeof(float) * G * Mg * h->Hp, 256);
    const size_t vbytes = sizeof(int) * (size_t)G * Mg;
    c->bytes = ragged ? kbytes + (size_t)round_up((int64_t)vbytes, 256) + sizeof(int) * (size_t)G : kbytes + vbytes;
    if (hipMalloc((void**)&c->mem, c->bytes) != hipSuccess) { delete c; return fail(h, FSMG_ERR_NOMEM, "hipMalloc(cache) failed"); }
    c->keys = (float*)c->mem;
    c->vals = (int*)(c->mem + kbytes);
    if (ragged) c->counts = (int*)(c->mem + c->bytes - sizeof(int) * (size_t)G);
    *out = c;
    return FSMG_OK;
}

// h->cat holds at least `bytes`: grown between calls, after a stream sync
int cat_reserve(fsmg_model* h, size_t bytes) {
    if (bytes <= h->cat_bytes) return FSMG_OK;
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->cat) hipFree(h->cat);
    h->cat = nullptr; h->cat_bytes = 0;
    if (hipMalloc((void**)&h->cat, bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(cache attention scratch) failed");
    h->cat_bytes = bytes;
    return FSMG_OK;
}

// The queries of an attention call sorted by group into tiles of CACHE_ATTEND_QT slots (one workgroup each): groups in increasing
// order, a group's queries in increasing id, the last tile of a group padded with -1.
struct Tiles {
    std::vector<int> slot_query, tile_group;
    int n_tiles() const { return (int)tile_group.size(); }
};
// keep(q): whether query q gets a slot at all (the scored positions of a *_masked call; the others get no slot and no tile)
template <class GroupOf, class Keep>
Tiles make_tiles(int n, int G, GroupOf&& group_of, Keep&& keep) {
    std::vector<int> count(G, 0), first(G + 1, 0);
    for (int q = 0; q < n; ++q)
        if (keep(q)) ++count[group_of(q)];
    for (int g = 0; g < G; ++g) first[g + 1] = first[g] + (count[g] + CACHE_ATTEND_QT - 1) / CACHE_ATTEND_QT;
    Tiles t;
    t.tile_group.resize(first[G]);
    t.slot_query.assign((size_t)first[G] * CACHE_ATTEND_QT, -1);
    std::vector<int> next(G);
    for (int g = 0; g < G; ++g) {
        next[g] = first[g] * CACHE_ATTEND_QT;
        for (int j = first[g]; j < first[g + 1]; ++j) t.tile_group[j] = g;
    }
    for (int q = 0; q < n; ++q)
        if (keep(q)) t.slot_query[next[group_of(q)]++] = q;
    return t;
}
template <class GroupOf>
Tiles make_tiles(int n, int G, GroupOf&& group_of) {
    return make_tiles(n, G, group_of, [](int) { return true; });
}

// The layout of an attention call in h->cat: [out n_theta x n floats | tiles | (raw form) targets n ints | queries n x Hp floats]
struct AttendScratch {
    float* out = nullptr; int* slot_query = nullptr; int* tile_group = nullptr; int* tgt = nullptr; float* Q = nullptr;
};
int attend_scratch(fsmg_model* h, int n, int n_theta, const Tiles& t, bool raw, AttendScratch* s) {
    Carver cv;
    const size_t o_out = cv.take(sizeof(float) * (size_t)n_theta * n);
    const size_t o_slot = cv.take(sizeof(int) * t.slot_query.size());
    const size_t o_grp = cv.take(sizeof(int) * t.tile_group.size());
    const size_t o_tgt = cv.take(raw ? sizeof(int) * (size_t)n : 0);
    const size_t o_q = cv.take(raw ? sizeof(float) * (size_t)n * h->Hp : 0);
    const int rc = cat_reserve(h, cv.off);
    if (rc != FSMG_OK) return rc;
    s->out = (float*)(h->cat + o_out); s->slot_query = (int*)(h->cat + o_slot); s->tile_group = (int*)(h->cat + o_grp);
    s->tgt = (int*)(h->cat + o_tgt); s->Q = (float*)(h->cat + o_q);
    return FSMG_OK;
}

// uploads the tiles and launches the attention kernel; the caller keeps `t` alive until the stream has been synchronised
int attend_launch(fsmg_model* h, const fsmg_cache_s* c, const Tiles& t, const AttendScratch& s, int n, const float* Q, int B,
                  const int* tgt, const float* thetas, int n_theta) {
    HIPCK(h, hipMemcpyAsync(s.slot_query, t.slot_query.data(), sizeof(int) * t.slot_query.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(s.tile_group, t.tile_group.data(), sizeof(int) * t.tile_group.size(), hipMemcpyHostToDevice, h->stream));
    CacheAttendArgs a{};
    a.keys = c->keys; a.vals = c->vals; a.count = c->counts; a.Mg = c->Mg; a.Hp = c->Hp;
    a.Q = Q; a.ldq = c->Hp; a.B = B; a.T = h->T; a.tgt = tgt;
    a.slot_query = s.slot_query; a.tile_group = s.tile_group; a.n_tiles = t.n_tiles(); a.n = n;
    for (int k = 0; k < n_theta; ++k) a.theta[k] = thetas[k];
    a.n_theta = n_theta; a.out = s.out;
    ScopedTimer tm(h, "cache_attend");
    HIPCK(h, launch_cache_attend(h->stream, a));
    return FSMG_OK;
}

// The layout of a self-cache attention call in h->cat: [out n_theta x n floats | row groups | (raw form) values n ints | vectors n x Hp floats]
struct SelfScratch {
    float* out = nullptr; int* row_group = nullptr; int* val = nullptr; float* V = nullptr;
};
int self_scratch(fsmg_model* h, int rows, int n, int n_theta, bool raw, SelfScratch* s) {
    Carver cv;
    const size_t o_out = cv.take(sizeof(float) * (size_t)n_theta * n);
    const size_t o_grp = cv.take(sizeof(int) * (size_t)rows);
    const size_t o_val = cv.take(raw ? sizeof(int) * (size_t)n : 0);
    const size_t o_v = cv.take(raw ? sizeof(float) * (size_t)n * h->Hp : 0);
    const int rc = cat_reserve(h, cv.off);
    if (rc != FSMG_OK) return rc;
    s->out = (float*)(h->cat + o_out); s->row_group = (int*)(h->cat + o_grp); s->val = (int*)(h->cat + o_val); s->V = (float*)(h->cat + o_v);
    return FSMG_OK;
}

// uploads the rows' groups (a support cache given) and launches the causal attention kernel over `rows` rows of T positions; `group`
// stays alive until the stream has been synchronised
int self_launch(fsmg_model* h, const fsmg_cache_s* c, const SelfScratch& s, int rows, int T, int W, const float* V, long long vs_r,
                long long vs_t, const int* val, long long ys_r, long long ys_t, const int32_t* group, const float* thetas, int n_theta) {
    CacheSelfArgs a{};
    if (c) {
        a.keys = c->keys; a.vals = c->vals; a.count = c->counts; a.Mg = c->Mg;
        if (group) {
            HIPCK(h, hipMemcpyAsync(s.row_group, group, sizeof(int) * (size_t)rows, hipMemcpyHostToDevice, h->stream));
            a.row_group = s.row_group;
        }
    }
    a.H = h->H; a.Hp = h->Hp;
    a.V = V; a.vs_r = vs_r; a.vs_t = vs_t; a.val = val; a.ys_r = ys_r; a.ys_t = ys_t;
    a.n_rows = rows; a.T = T; a.W = W;
    for (int k = 0; k < n_theta; ++k) a.theta[k] = thetas[k];
    a.n_theta = n_theta; a.out = s.out;
    ScopedTimer tm(h, "cache_attend_self");
    HIPCK(h, launch_cache_attend_self(h->stream, a));
    return FSMG_OK;
}

int check_self_config(fsmg_model* h, const fsmg_cache_self_config* sc) {
    const int rc = check_config_header(h, sc, "fsmg_cache_self_config", FSMG_CACHE_SELF_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (sc->window < 1) return fail(h, FSMG_ERR_INVALID, "fsmg_cache_self_config.window must be >= 1");
    return FSMG_OK;
}

bool thetas_ok(const float* thetas, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(thetas[k]) || thetas[k] < 0.0f) return false;
    return true;
}

// the n group ids of a call against a cache of G groups (null: every row in group 0)
int check_group_ids(fsmg_model* h, const int32_t* group, int64_t n, int G) {
    if (group)
        for (int64_t i = 0; i < n; ++i)
            if (group[i] < 0 || group[i] >= G) return fail(h, FSMG_ERR_INVALID, "group id outside [0, groups of the cache)");
    return FSMG_OK;
}

int check_build_config(fsmg_model* h, const fsmg_cache_config* c, const int32_t* tokens, fsmg_cache* out) {
    if (!c || !out) return fail(h, FSMG_ERR_INVALID, "null fsmg_cache_config / out");
    const int rc = check_config_header(h, c, "fsmg_cache_config", FSMG_CACHE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (c->n_rows < 1 || c->n_rows > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n_rows must be in [1, 2^20]");
    if (c->n_groups < 1 || c->n_rows % c->n_groups != 0) return fail(h, FSMG_ERR_INVALID, "n_groups must be >= 1 and divide n_rows");
    if (c->tokens_on_device != 0 && c->tokens_on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (c->pass_rows < 0 || c->pass_rows > 1024) return fail(h, FSMG_ERR_INVALID, "pass_rows must be 0 or in [1, 1024]");
    if (!tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    return check_cache_size(h, c->n_groups, (int64_t)(c->n_rows / c->n_groups) * h->T);
}

// fsmg_cache_build's work behind the argument checks; with `len` (host [R], checked) fsmg_cache_build_masked's: the same passes, the
// compacting fill behind each, a ragged cache of n_g = the group's lengths summed
int build_core(fsmg_model* h, const fsmg_cache_config* c, const int32_t* tokens, fsmg_cache_s** out, const int32_t* len = nullptr) {
    const int R = c->n_rows, T = h->T;
    const int P = c->pass_rows > 0 ? c->pass_rows : FSMG_SCORE_PASS_ROWS;
    int rc;
    if (!c->tokens_on_device && (rc = check_host_tokens(h, tokens, (size_t)R * T)) != FSMG_OK) return rc;
    if ((rc = ensure_scratch(h, std::min(R, P))) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    fsmg_cache_s* cache = nullptr;
    const int rpg = R / c->n_groups, Mg = rpg * T;
    if ((rc = alloc_cache(h, c->n_groups, Mg, &cache, len != nullptr)) != FSMG_OK) return rc;
    std::vector<int> dst;               // row r's first entry in the flat [G * Mg] entries; alive until the last pass is synchronised
    int *d_len = nullptr, *d_dst = nullptr;
    if (len) {
        cache->n_g.assign((size_t)c->n_groups, 0);
        dst.resize((size_t)R);
        for (int r = 0; r < R; ++r) {
            int& n = cache->n_g[(size_t)(r / rpg)];
            dst[r] = (r / rpg) * Mg + n;
            n += len[r];
        }
        // a pass's lengths and offsets in h->cat; every slot zero once, so that what lies behind a group's count reads back as zeros
        Carver cv;
        const size_t o_len = cv.take(sizeof(int) * (size_t)std::min(R, P)), o_dst = cv.take(sizeof(int) * (size_t)std::min(R, P));
        rc = cat_reserve(h, cv.off);
        hipError_t e = hipSuccess;
        if (rc == FSMG_OK) e = hipMemsetAsync(cache->mem, 0, cache->bytes, h->stream);
        if (rc == FSMG_OK && e == hipSuccess)
            e = hipMemcpyAsync(cache->counts, cache->n_g.data(), sizeof(int) * cache->n_g.size(), hipMemcpyHostToDevice, h->stream);
        if (rc == FSMG_OK && e != hipSuccess) rc = fail(h, FSMG_ERR_HIP, std::string("ragged cache setup: ") + hipGetErrorString(e));
        if (rc != FSMG_OK) { hipStreamSynchronize(h->stream); free_cache(cache); return rc; }
        d_len = (int*)(h->cat + o_len); d_dst = (int*)(h->cat + o_dst);
    }
    rc = run_passes(
        h, tokens, R, P, c->tokens_on_device,
        [&](int r0, int B) -> int {
            const int r = run_graphed(h, "cb:" + std::to_string(B), [&]() -> int {
                const int rr = token_prep(h, 0, B);
                return rr == FSMG_OK ? forward(h, B, B, 1, nullptr, false, HEAD_NONE) : rr;
            });
            if (r != FSMG_OK) return r;
            // rows r0 .. r0 + B - 1 of the cache's [rows][T] entries: a pass repeated after a time-out overwrites what it wrote
            if (!len) {
                HIPCK(h, launch_cache_fill(h->stream, h->Hs[h->L - 1] + (size_t)B * h->Hp, h->Y, B, T, h->H, h->Hp, r0, cache->keys, cache->vals));
                return FSMG_OK;
            }
            // the compacting fill, outside the graph as the plain one: the same entries on a repeated pass
            HIPCK(h, hipMemcpyAsync(d_len, len + r0, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
            HIPCK(h, hipMemcpyAsync(d_dst, dst.data() + r0, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, h->stream));
            HIPCK(h, launch_cache_fill_len(h->stream, h->Hs[h->L - 1] + (size_t)B * h->Hp, h->Y, B, T, h->H, h->Hp, d_len, d_dst, cache->keys,
                                           cache->vals));
            return FSMG_OK;
        },
        [](int, int) { return FSMG_OK; });          // (nothing comes back but the error word)
    if (rc != FSMG_OK) { hipStreamSynchronize(h->stream); free_cache(cache); return rc; }
    *out = cache;
    return FSMG_OK;
}

int check_score_config(fsmg_model* h, const fsmg_cache_s* cache, const fsmg_cache_score_config* c, const int32_t* tokens,
                       const int32_t* group, const void* const outs[4]) {
    const int rc = check_config_header(h, c, "fsmg_cache_score_config", FSMG_CACHE_SCORE_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (c->n_rows < 1 || c->n_rows > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n_rows must be in [1, 2^20]");
    if (c->tokens_on_device != 0 && c->tokens_on_device != 1) return fail(h, FSMG_ERR_INVALID, "tokens_on_device must be 0 or 1");
    if (c->nll_first < 0 || c->nll_first >= h->T || c->nll_count < 0 || (int64_t)c->nll_first + c->nll_count > h->T)
        return fail(h, FSMG_ERR_INVALID, "nll_first must be in [0, max_len) and nll_first + nll_count <= max_len");
    if (c->pass_rows < 0 || c->pass_rows > 1024) return fail(h, FSMG_ERR_INVALID, "pass_rows must be 0 or in [1, 1024]");
    if (c->n_theta < 1 || c->n_theta > FSMG_CACHE_MAX_THETA) return fail(h, FSMG_ERR_INVALID, "n_theta must be in [1, 8]");
    if (!thetas_ok(c->thetas, c->n_theta)) return fail(h, FSMG_ERR_INVALID, "every theta must be finite and >= 0");
    if (c->n_lambda < 1 || c->n_lambda > FSMG_CACHE_MAX_LAMBDA) return fail(h, FSMG_ERR_INVALID, "n_lambda must be in [1, 16]");
    for (int j = 0; j < c->n_lambda; ++j)
        if (!(c->lambdas[j] >= 0.0f && c->lambdas[j] <= 1.0f)) return fail(h, FSMG_ERR_INVALID, "every lambda must lie in [0, 1]");
    if (!tokens) return fail(h, FSMG_ERR_INVALID, "null tokens");
    if (!outs[0] && !outs[1] && !outs[2] && !outs[3]) return fail(h, FSMG_ERR_INVALID, "every output is null");
    if (cache->H != h->H || cache->Hp != h->Hp) return fail(h, FSMG_ERR_INVALID, "the cache's hidden size is not the handle's");
    return check_group_ids(h, group, c->n_rows, cache->G);
}

// fsmg_cache_score's work behind the argument checks; with `self` fsmg_cache_self_score's: the row's own history joins the set (the
// causal kernel instead of k_cache_attend), `cache` may then be null, and a position whose set is empty keeps the model's log-prob
int score_core(fsmg_model* h, const fsmg_cache_s* cache, const fsmg_cache_score_config* c, const int32_t* tokens, const int32_t* group,
               float* out_logprob, float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll,
               const fsmg_cache_self_config* self = nullptr, const int32_t* len = nullptr) {
    // `len` (host [R], checked): the *_masked calls.  Position t of row r is scored iff t < len[r]; the passes are the same launches,
    // the support attention gets tiles over the scored queries only, and every output is +0 behind a song's end.
    const int R = c->n_rows, T = h->T, NT = c->n_theta, NL = c->n_lambda;
    const int P = c->pass_rows > 0 ? c->pass_rows : FSMG_SCORE_PASS_ROWS;
    const size_t RT = (size_t)R * T;
    int rc;
    if (!c->tokens_on_device && (rc = check_host_tokens(h, tokens, RT)) != FSMG_OK) return rc;
    if ((rc = ensure_scratch(h, std::min(R, P))) != FSMG_OK) return rc;
    if ((rc = ensure_khf(h)) != FSMG_OK) return rc;
    // the mixture and the row NLL are host work over the two device outputs: those come to the host whether asked for or not
    const bool want_mix = out_logprob != nullptr || out_row_nll != nullptr;
    const bool want_pc = want_mix || out_cache_prob != nullptr, want_lp = want_mix || out_lstm_logprob != nullptr;
    std::vector<float> lp_own, pc_own, mix_own;
    float* lp_host = out_lstm_logprob;
    float* pc_host = out_cache_prob;
    if (want_lp && !lp_host) { lp_own.resize(RT); lp_host = lp_own.data(); }
    if (want_pc && !pc_host) { pc_own.resize(RT * NT); pc_host = pc_own.data(); }
    Tiles tiles;                        // a pass's attention scratch, from its launches to its read-back
    AttendScratch as;
    SelfScratch ss;
    rc = run_passes(
        h, tokens, R, P, c->tokens_on_device,
        [&](int r0, int B) -> int {
            const int n = B * T;
            int r;
            if (want_pc && self) {
                if ((r = self_scratch(h, B, n, NT, false, &ss)) != FSMG_OK) return r;
                as.out = ss.out;
            } else if (want_pc) {       // query q = b * T + t of the pass, in its row's group
                tiles = make_tiles(n, cache->G, [&](int q) { return group ? group[r0 + q / T] : 0; },
                                   [&](int q) { return !len || q % T < len[r0 + q / T]; });
                if ((r = attend_scratch(h, n, NT, tiles, false, &as)) != FSMG_OK) return r;
            }
            // fsmg_score's pass with the log-prob as its one output (the same graph key: the same launches)
            r = run_graphed(h, "sc:" + std::to_string(B) + ":1", [&]() -> int {
                int rr = token_prep(h, 0, B);
                if (rr == FSMG_OK) rr = forward(h, B, B, 1, nullptr, false, HEAD_LOGITS);
                if (rr != FSMG_OK) return rr;
                ScopedTimer tm(h, "ce");
                HIPCK(h, launch_score_rows(h->stream, h->logits, h->V1p, n, h->V1, h->Y, B, T, h->score_out, nullptr, nullptr, nullptr));
                return FSMG_OK;
            });
            if (r != FSMG_OK || !want_pc) return r;
            if (len && !self) HIPCK(h, hipMemsetAsync(as.out, 0, sizeof(float) * (size_t)NT * n, h->stream));   // the queries without a tile
            if (!self) return attend_launch(h, cache, tiles, as, n, h->Hs[h->L - 1], B, h->Y, c->thetas, NT);
            // row b's vector t: slot t + 1 of the time-major top-layer states; its value t: Y[t][b]
            return self_launch(h, cache, ss, B, T, self->window, h->Hs[h->L - 1] + (size_t)B * h->Hp, h->Hp, (long long)B * h->Hp, h->Y, 1, B,
                               group ? group + r0 : nullptr, c->thetas, NT);
        },
        [&](int r0, int B) -> int {
            const size_t o = (size_t)r0 * T, n = (size_t)B * T;
            if (want_lp) HIPCK(h, hipMemcpyAsync(lp_host + o, h->score_out, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
            if (want_pc)
                for (int k = 0; k < NT; ++k)
                    HIPCK(h, hipMemcpyAsync(pc_host + k * RT + o, as.out + (size_t)k * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
            return FSMG_OK;
        });
    if (rc != FSMG_OK) return rc;
    auto clear_tail = [&](float* plane) {           // +0 at the positions behind each song's end
        for (int r = 0; r < R; ++r)
            for (size_t i = (size_t)r * T + len[r]; i < (size_t)(r + 1) * T; ++i) plane[i] = 0.0f;
    };
    if (len && want_lp) clear_tail(lp_host);
    if (len && want_pc)
        for (int k = 0; k < NT; ++k) clear_tail(pc_host + k * RT);
    if (!want_mix) return FSMG_OK;
    float* mix = out_logprob;
    if (!mix) { mix_own.resize(RT); mix = mix_own.data(); }            // (row NLL alone: one (theta, lambda) plane at a time)
    for (int k = 0; k < NT; ++k)
        for (int j = 0; j < NL; ++j) {
            const double lam = (double)c->lambdas[j];
            const double l1m = std::log1p(-lam), ll = std::log(lam);
            float* plane = out_logprob ? mix + ((size_t)k * NL + j) * RT : mix;
            const float* pc = pc_host + k * RT;
            for (size_t i = 0; i < RT; ++i) plane[i] = mix_logprob(lp_host[i], pc[i], l1m, ll);
            if (self && !cache)         // position 0 of a row has an empty set: the model alone, at every lambda
                for (size_t i = 0; i < RT; i += T) plane[i] = lp_host[i];
            if (len) clear_tail(plane);
            if (out_row_nll && len) row_nll_masked(plane, R, T, c->nll_first, c->nll_count, len, out_row_nll + ((size_t)k * NL + j) * R);
            else if (out_row_nll) row_nll(plane, R, T, c->nll_first, c->nll_count, out_row_nll + ((size_t)k * NL + j) * R);
        }
    return FSMG_OK;
}

}  // namespace

// ---- cache-conditioned generation: the cache side (the decode driver in api_decode.hip calls these)
constexpr int64_t SELF_GEN_MAX_KEY_FLOATS = 1LL << 29;   // R * NP * Hp of one call (2 GiB of own keys)

// what cache_gen_check and cache_self_gen_check share: the config, then -- with a support cache (it may be absent only where
// `need_cache` is false) -- the cache against the handle, the R * Mg limit, the group ids and the rows' tiles
static int gen_check(fsmg_model* h, fsmg_cache cache, bool need_cache, const fsmg_cache_gen_config* cc, const int32_t* group, int64_t R,
                     CacheGen* cg) {
    fsmg_cache_s* c = nullptr;
    if ((cache || need_cache) && !(c = find_cache(h, cache))) return FSMG_ERR_INVALID;
    int rc = check_config_header(h, cc, "fsmg_cache_gen_config", FSMG_CACHE_GEN_CONFIG_VERSION);
    if (rc != FSMG_OK) return rc;
    if (!thetas_ok(&cc->theta, 1)) return fail(h, FSMG_ERR_INVALID, "theta must be finite and >= 0");
    if (!(cc->lambda >= 0.0f && cc->lambda <= 1.0f)) return fail(h, FSMG_ERR_INVALID, "lambda must lie in [0, 1]");
    if (R < 1 || R > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "the row count must be in [1, 2^20]");
    cg->c = c; cg->theta = cc->theta; cg->lambda = cc->lambda;
    cg->R = (int)R; cg->ldl = (int)round_up(h->V1, 64);
    if (!c) return FSMG_OK;
    if (c->H != h->H || c->Hp != h->Hp) return fail(h, FSMG_ERR_INVALID, "the cache's hidden size is not the handle's");
    if (R * c->Mg > CACHE_GEN_MAX_SCORES) return fail(h, FSMG_ERR_INVALID, "rows * entries_per_group must be <= 2^26");
    if ((rc = check_group_ids(h, group, R, c->G)) != FSMG_OK) return rc;
    Tiles t = make_tiles((int)R, c->G, [&](int q) { return group ? group[q] : 0; });
    cg->slot_query = std::move(t.slot_query);
    cg->tile_group = std::move(t.tile_group);
    cg->row_group.resize((size_t)R);
    for (int64_t r = 0; r < R; ++r) cg->row_group[r] = group ? group[r] : 0;
    return FSMG_OK;
}

int cache_gen_check(fsmg_model* h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const int32_t* group, int64_t R, CacheGen* cg) {
    return gen_check(h, cache, true, cc, group, R, cg);
}

int cache_self_gen_check(fsmg_model* h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                         const int32_t* group, int64_t R, int64_t NP, bool raw, CacheGen* cg) {
    int rc = gen_check(h, cache, false, cc, group, R, cg);
    if (rc == FSMG_OK) rc = check_self_config(h, sc);
    if (rc != FSMG_OK) return rc;
    if (NP < 1) NP = 1;
    if (R * NP * h->Hp > SELF_GEN_MAX_KEY_FLOATS)
        return fail(h, FSMG_ERR_INVALID, "rows * (primer_len + num) * Hp (Hp the padded hidden size) must be <= 2^29");
    cg->W = sc->window; cg->Hp = h->Hp; cg->NP = (int)NP; cg->ldo = (int)std::min<int64_t>(sc->window, NP); cg->raw = raw;
    if (R * cg->ldo > CACHE_GEN_MAX_SCORES) return fail(h, FSMG_ERR_INVALID, "rows * min(window, positions) must be <= 2^26");
    return FSMG_OK;
}

int ensure_value_index(fsmg_model* h, fsmg_cache_s* c) {
    if (c->idx_mem) return FSMG_OK;
    const size_t G = c->G, Mg = c->Mg, n = G * Mg;
    std::vector<int> vals(n);
    HIPCK(h, hipMemcpyAsync(vals.data(), c->vals, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    // one host block [order | seg_beg | seg_end | seg_val (G * Mg each) | n_seg | n_long (G each)], the device layout
    std::vector<int> idx(4 * n + 2 * G, 0);
    int* order = idx.data();
    int* seg_beg = order + n;
    int* seg_end = seg_beg + n;
    int* seg_val = seg_end + n;
    int* n_seg = seg_val + n;
    int* n_long = n_seg + G;
    std::vector<int> beg;                               // a group's segment starts in value order
    for (size_t g = 0; g < G; ++g) {
        const int* v = vals.data() + g * Mg;
        int* o = order + g * Mg;
        const size_t ng = (size_t)c->entries((int)g);       // the entries that exist: the slots behind them are in no segment
        for (size_t i = 0; i < ng; ++i) o[i] = (int)i;
        std::stable_sort(o, o + ng, [&](int x, int y) { return v[x] < v[y]; });
        beg.clear();
        for (size_t j = 0; j < ng; ++j)
            if (j == 0 || v[o[j]] != v[o[j - 1]]) beg.push_back((int)j);
        beg.push_back((int)ng);
        // the segments longer than CACHE_MIX_SHORT first (a wave each), then the others (a thread each), value order inside both
        int ns = 0;
        for (int pass = 0; pass < 2; ++pass) {
            for (size_t s = 0; s + 1 < beg.size(); ++s) {
                if ((beg[s + 1] - beg[s] > CACHE_MIX_SHORT) != (pass == 0)) continue;
                seg_beg[g * Mg + ns] = beg[s]; seg_end[g * Mg + ns] = beg[s + 1]; seg_val[g * Mg + ns] = v[o[beg[s]]];
                ++ns;
            }
            if (pass == 0) n_long[g] = ns;
        }
        n_seg[g] = ns;
    }
    const size_t bytes = sizeof(int) * idx.size();
    char* mem = nullptr;
    if (hipMalloc((void**)&mem, bytes) != hipSuccess) return fail(h, FSMG_ERR_NOMEM, "hipMalloc(cache value index) failed");
    hipError_t e = hipMemcpyAsync(mem, idx.data(), bytes, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);           // the host vector goes out of scope
    if (e != hipSuccess) { hipFree(mem); return fail(h, FSMG_ERR_HIP, std::string("value index upload: ") + hipGetErrorString(e)); }
    c->idx_mem = mem;
    c->order = (int*)mem;
    c->seg_beg = c->order + n;
    c->seg_end = c->seg_beg + n;
    c->seg_val = c->seg_end + n;
    c->n_seg = c->seg_val + n;
    c->n_long = c->n_seg + G;
    c->bytes += bytes;
    return FSMG_OK;
}

namespace {
// [D R * Mg doubles | pc R * ldl floats | slot_query | tile_group | row_group], each 256-byte aligned
struct CacheGenLayout { size_t o_D, o_pc, o_slot, o_tile, o_row, o_keys, o_D2, o_pm, o_len, o_val, total; };
CacheGenLayout cache_gen_layout(const CacheGen& cg) {
    Carver cv;
    CacheGenLayout l{};
    l.o_D = cv.take(sizeof(double) * (size_t)cg.R * (cg.c ? cg.c->Mg : 0));
    l.o_pc = cv.take(sizeof(float) * (size_t)cg.R * cg.ldl);
    l.o_slot = cv.take(sizeof(int) * cg.slot_query.size());
    l.o_tile = cv.take(sizeof(int) * cg.tile_group.size());
    l.o_row = cv.take(sizeof(int) * cg.row_group.size());
    if (cg.W > 0) {         // (behind everything else: without a self-cache the layout is what it was)
        l.o_keys = cv.take(sizeof(float) * (size_t)cg.R * cg.NP * cg.Hp);
        l.o_D2 = cv.take(sizeof(double) * (size_t)cg.R * cg.ldo);
        l.o_pm = cv.take(sizeof(double) * (size_t)cg.R * cg.ldl);
        l.o_len = cv.take(cg.raw ? sizeof(int) * (size_t)cg.R : 0);
        l.o_val = cv.take(cg.raw ? sizeof(int) * (size_t)cg.R * cg.NP : 0);
    }
    l.total = cv.off;
    return l;
}
}  // namespace

size_t cache_gen_bytes(const fsmg_model*, const CacheGen& cg) { return cache_gen_layout(cg).total; }

int cache_gen_place(fsmg_model* h, CacheGen& cg, char* base) {
    const CacheGenLayout l = cache_gen_layout(cg);
    cg.D = (double*)(base + l.o_D); cg.pc = (float*)(base + l.o_pc);
    cg.d_slot_query = (int*)(base + l.o_slot); cg.d_tile_group = (int*)(base + l.o_tile); cg.d_row_group = (int*)(base + l.o_row);
    if (cg.W > 0) {
        cg.own_keys = (float*)(base + l.o_keys); cg.D2 = (double*)(base + l.o_D2); cg.pm = (double*)(base + l.o_pm);
        cg.d_len = (int*)(base + l.o_len); cg.d_val = (int*)(base + l.o_val);
    }
    if (!cg.c) return FSMG_OK;          // no support entries: no tiles
    HIPCK(h, hipMemcpyAsync(cg.d_slot_query, cg.slot_query.data(), sizeof(int) * cg.slot_query.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(cg.d_tile_group, cg.tile_group.data(), sizeof(int) * cg.tile_group.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(cg.d_row_group, cg.row_group.data(), sizeof(int) * cg.row_group.size(), hipMemcpyHostToDevice, h->stream));
    return FSMG_OK;
}

int cache_self_file(fsmg_model* h, const CacheGen& cg, const float* h_out, int p) {
    ScopedTimer tm(h, "self_file");
    HIPCK(h, launch_self_file(h->stream, h_out, cg.R, h->H, h->Hp, cg.own_keys, cg.NP, p));
    return FSMG_OK;
}

// stage one over the support entries: the rows' queries Q against their groups' keys into cg.D
static int scores_launch(fsmg_model* h, const CacheGen& cg, const float* Q) {
    const fsmg_cache_s* c = cg.c;
    CacheScoresArgs sa{};
    sa.keys = c->keys; sa.count = c->counts; sa.Mg = c->Mg; sa.Hp = c->Hp; sa.Q = Q; sa.ldq = c->Hp;
    sa.slot_query = cg.d_slot_query; sa.tile_group = cg.d_tile_group; sa.n_tiles = (int)cg.tile_group.size(); sa.D = cg.D;
    ScopedTimer tm(h, "cache_scores");
    HIPCK(h, launch_cache_scores(h->stream, sa));
    return FSMG_OK;
}

// stage two's arguments; without a support cache Mg stays 0 and D, row_group and the value index stay null
static CacheMixArgs mix_args(const fsmg_model* h, const CacheGen& cg, float* logits, float* out_lse) {
    const double lam = (double)cg.lambda;
    CacheMixArgs ma{};
    ma.logits = logits; ma.ldl = cg.ldl; ma.ncols = h->V1; ma.pc = cg.pc; ma.out_lse = out_lse;
    if (const fsmg_cache_s* c = cg.c) {
        ma.D = cg.D; ma.Mg = c->Mg; ma.count = c->counts; ma.row_group = cg.d_row_group;
        ma.order = c->order; ma.seg_beg = c->seg_beg; ma.seg_end = c->seg_end; ma.seg_val = c->seg_val;
        ma.n_seg = c->n_seg; ma.n_long = c->n_long;
    }
    ma.u = (double)cg.theta * CA_LOG2E; ma.log1m_lambda = std::log1p(-lam); ma.log_lambda = std::log(lam); ma.mix = cg.lambda > 0.0f;
    return ma;
}

int cache_self_step(fsmg_model* h, const CacheGen& cg, int len, const float* Q, float* logits, const int* val, int ldv, float* out_lse) {
    int rc;
    if (cg.c && (rc = scores_launch(h, cg, Q)) != FSMG_OK) return rc;
    const int* row_len = cg.raw ? cg.d_len : nullptr;
    SelfScoresArgs ss{};
    ss.own_keys = cg.own_keys; ss.NP = cg.NP; ss.Hp = h->Hp; ss.Q = Q; ss.ldq = h->Hp;
    ss.row_len = row_len; ss.len = len; ss.W = cg.W; ss.D2 = cg.D2; ss.ldo = cg.ldo; ss.R = cg.R;
    {
        ScopedTimer tm(h, "self_scores");
        HIPCK(h, launch_self_scores(h->stream, ss));
    }
    CacheMixSelfArgs ma{};
    ma.m = mix_args(h, cg, logits, out_lse);
    ma.D2 = cg.D2; ma.ldo = cg.ldo; ma.val = val; ma.ldv = ldv; ma.row_len = row_len; ma.len = len; ma.W = cg.W; ma.pm = cg.pm;
    ScopedTimer tm(h, "cache_mix_self");
    HIPCK(h, launch_cache_mix_self(h->stream, cg.R, ma));
    return FSMG_OK;
}

int cache_gen_step(fsmg_model* h, const CacheGen& cg, const float* Q, float* logits, float* out_lse) {
    const int rc = scores_launch(h, cg, Q);
    if (rc != FSMG_OK) return rc;
    ScopedTimer tm(h, "cache_mix");
    HIPCK(h, launch_cache_mix(h->stream, cg.R, mix_args(h, cg, logits, out_lse)));
    return FSMG_OK;
}

namespace {
// what fsmg_cache_self_distribution adds to fsmg_cache_distribution: per query up to S own entries, self_len[q] of them filed
struct SelfEntries {
    const fsmg_cache_self_config* sc;
    const float* keys; const int32_t* values; const int32_t* len; int32_t S;
};

// fsmg_cache_distribution, and with `self` fsmg_cache_self_distribution (the cache may then be null)
int distribution(fsmg_model* h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const SelfEntries* self, int32_t n, const float* queries,
                 const float* logits, const int32_t* group, float* out_cache_prob, float* out_logprob, float* out_lse) {
    if ((cache || !self) && !find_cache(h, cache)) return FSMG_ERR_INVALID;
    if (n < 1 || n > (1 << 20)) return fail(h, FSMG_ERR_INVALID, "n must be in [1, 2^20]");
    if (!self && (!queries || !logits)) return fail(h, FSMG_ERR_INVALID, "null queries / logits");
    if (self && (!queries || !logits || !self->len)) return fail(h, FSMG_ERR_INVALID, "null queries / logits / self_len");
    const int S = self ? self->S : 0;
    if (S < 0 || (S > 0 && (!self->keys || !self->values))) return fail(h, FSMG_ERR_INVALID, "S must be >= 0, with self_keys and self_values when S > 0");
    if (!out_cache_prob && !out_logprob && !out_lse) return fail(h, FSMG_ERR_INVALID, "every output is null");
    CacheGen cg;
    int rc = self ? cache_self_gen_check(h, cache, cc, self->sc, cache ? group : nullptr, n, S, true, &cg) : cache_gen_check(h, cache, cc, group, n, &cg);
    if (rc != FSMG_OK) return rc;
    if (self) {
        for (int i = 0; i < n; ++i)
            if (self->len[i] < 0 || self->len[i] > S) return fail(h, FSMG_ERR_INVALID, "self_len outside [0, S]");
        for (size_t i = 0; i < (size_t)n * S; ++i)
            if (self->values[i] < 0 || self->values[i] >= h->V1) return fail(h, FSMG_ERR_TOKEN_RANGE, "own value outside [0, input_size]");
    }
    BEGIN_CALL(h);
    if (cg.c && (rc = ensure_value_index(h, const_cast<fsmg_cache_s*>(cg.c))) != FSMG_OK) return rc;
    // [cache_gen's block | queries n x Hp | logits n x ldl | lse n]
    const int Hp = h->Hp, ldl = cg.ldl, V1 = h->V1, NP = cg.NP;
    Carver cv;
    cv.take(cache_gen_bytes(h, cg));
    const size_t o_q = cv.take(sizeof(float) * (size_t)n * Hp);
    const size_t o_z = cv.take(sizeof(float) * (size_t)n * ldl);
    const size_t o_lse = cv.off;
    if ((rc = gen_reserve(h, o_lse + sizeof(float) * (size_t)n)) != FSMG_OK) return rc;
    float* d_q = (float*)(h->gen + o_q);
    float* d_z = (float*)(h->gen + o_z);
    float* d_lse = (float*)(h->gen + o_lse);
    std::vector<float> qp((size_t)n * Hp, 0.0f), kp(self ? (size_t)n * NP * Hp : 0, 0.0f);       // the pad units are exact zeros
    std::vector<int> vp(self ? (size_t)n * NP : 0, 0);
    for (int q = 0; q < n; ++q) {
        std::memcpy(qp.data() + (size_t)q * Hp, queries + (size_t)q * h->H, sizeof(float) * h->H);
        for (int e = 0; e < S; ++e) {
            std::memcpy(kp.data() + ((size_t)q * NP + e) * Hp, self->keys + ((size_t)q * S + e) * h->H, sizeof(float) * h->H);
            vp[(size_t)q * NP + e] = self->values[(size_t)q * S + e];
        }
    }
    auto run = [&]() -> int {
        int r = cache_gen_place(h, cg, h->gen);
        if (r != FSMG_OK) return r;
        HIPCK(h, hipMemcpyAsync(d_q, qp.data(), sizeof(float) * qp.size(), hipMemcpyHostToDevice, h->stream));
        if (self) {
            HIPCK(h, hipMemcpyAsync(cg.own_keys, kp.data(), sizeof(float) * kp.size(), hipMemcpyHostToDevice, h->stream));
            HIPCK(h, hipMemcpyAsync(cg.d_val, vp.data(), sizeof(int) * vp.size(), hipMemcpyHostToDevice, h->stream));
            HIPCK(h, hipMemcpyAsync(cg.d_len, self->len, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        }
        HIPCK(h, hipMemcpy2DAsync(d_z, sizeof(float) * ldl, logits, sizeof(float) * V1, sizeof(float) * V1, n, hipMemcpyHostToDevice, h->stream));
        r = self ? cache_self_step(h, cg, 0, d_q, d_z, cg.d_val, NP, d_lse) : cache_gen_step(h, cg, d_q, d_z, d_lse);
        if (r != FSMG_OK) return r;
        if (out_cache_prob)
            HIPCK(h, hipMemcpy2DAsync(out_cache_prob, sizeof(float) * V1, cg.pc, sizeof(float) * ldl, sizeof(float) * V1, n, hipMemcpyDeviceToHost, h->stream));
        if (out_logprob)
            HIPCK(h, hipMemcpy2DAsync(out_logprob, sizeof(float) * V1, d_z, sizeof(float) * ldl, sizeof(float) * V1, n, hipMemcpyDeviceToHost, h->stream));
        if (out_lse) HIPCK(h, hipMemcpyAsync(out_lse, d_lse, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        return FSMG_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(h->stream);       // the host vectors go out of scope
    if (rc == FSMG_OK && e != hipSuccess) return fail(h, FSMG_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}
}  // namespace

}  // namespace fsmg_host

// =========================================================================== C ABI
extern "C" {

int fsmg_cache_build(fsmg_handle h, const fsmg_cache_config* c, const int32_t* tokens, fsmg_cache* out) {
    if (!h) return FSMG_ERR_INVALID;
    const int rc0 = check_build_config(h, c, tokens, out);
    if (rc0 != FSMG_OK) return rc0;
    BEGIN_CALL(h);
    fsmg_cache_s* cache = nullptr;
    const int rc = build_core(h, c, tokens, &cache);
    if (rc != FSMG_OK) return rc;
    h->caches.push_back(cache);
    *out = cache;
    return FSMG_OK;
}

int fsmg_cache_create_from(fsmg_handle h, int32_t n_groups, int32_t entries_per_group, const float* keys, const int32_t* values,
                           fsmg_cache* out) {
    if (!h) return FSMG_ERR_INVALID;
    if (!keys || !values || !out) return fail(h, FSMG_ERR_INVALID, "null keys / values / out");
    int rc = check_cache_size(h, n_groups, entries_per_group);
    if (rc != FSMG_OK) return rc;
    const size_t n = (size_t)n_groups * entries_per_group;
    for (size_t i = 0; i < n; ++i)
        if (values[i] < 0 || values[i] >= h->V1) return fail(h, FSMG_ERR_TOKEN_RANGE, "cache value outside [0, input_size]");
    BEGIN_CALL(h);
    fsmg_cache_s* c = nullptr;
    if ((rc = alloc_cache(h, n_groups, entries_per_group, &c)) != FSMG_OK) return rc;
    std::vector<float> kp(n * h->Hp, 0.0f);             // the pad units are exact zeros
    for (size_t i = 0; i < n; ++i) std::memcpy(kp.data() + i * h->Hp, keys + i * h->H, sizeof(float) * h->H);
    hipError_t e = hipMemcpyAsync(c->keys, kp.data(), sizeof(float) * kp.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->vals, values, sizeof(int) * n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);           // the host vector goes out of scope
    if (e != hipSuccess) { free_cache(c); return fail(h, FSMG_ERR_HIP, std::string("cache upload: ") + hipGetErrorString(e)); }
    h->caches.push_back(c);
    *out = c;
    return FSMG_OK;
}

int fsmg_cache_get(fsmg_handle h, fsmg_cache cache, float* keys, int32_t* values) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = find_cache(h, cache);
    if (!c) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    const size_t n = (size_t)c->G * c->Mg;
    std::vector<float> kp(keys ? n * c->Hp : 0);
    if (keys) HIPCK(h, hipMemcpyAsync(kp.data(), c->keys, sizeof(float) * kp.size(), hipMemcpyDeviceToHost, h->stream));
    if (values) HIPCK(h, hipMemcpyAsync(values, c->vals, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (keys)
        for (size_t i = 0; i < n; ++i) std::memcpy(keys + i * c->H, kp.data() + i * c->Hp, sizeof(float) * c->H);   // the padded units stay inside
    return FSMG_OK;
}

int fsmg_cache_info(fsmg_handle h, fsmg_cache cache, int64_t out[4]) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = find_cache(h, cache);
    if (!c) return FSMG_ERR_INVALID;
    if (!out) return fail(h, FSMG_ERR_INVALID, "null out");
    out[0] = c->G; out[1] = c->Mg; out[2] = c->H; out[3] = (int64_t)c->bytes;
    return FSMG_OK;
}

int fsmg_cache_destroy(fsmg_handle h, fsmg_cache cache) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = find_cache(h, cache);
    if (!c) return FSMG_ERR_INVALID;
    BEGIN_CALL(h);
    HIPCK(h, hipStreamSynchronize(h->stream));      // nothing in flight reads it
    h->caches.erase(std::find(h->caches.begin(), h->caches.end(), c));
    free_cache(c);
    return FSMG_OK;
}

int fsmg_cache_attend(fsmg_handle h, fsmg_cache cache, int32_t n, const float* queries, const int32_t* targets, const int32_t* group,
                      const float* thetas, int32_t n_theta, float* out_prob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = find_cache(h, cache);
    if (!c) return FSMG_ERR_INVALID;
    if (n < 1 || n > (1 << 22)) return fail(h, FSMG_ERR_INVALID, "n must be in [1, 2^22]");
    if (!queries || !targets || !thetas || !out_prob) return fail(h, FSMG_ERR_INVALID, "null queries / targets / thetas / out_prob");
    if (n_theta < 1 || n_theta > FSMG_CACHE_MAX_THETA) return fail(h, FSMG_ERR_INVALID, "n_theta must be in [1, 8]");
    if (!thetas_ok(thetas, n_theta)) return fail(h, FSMG_ERR_INVALID, "every theta must be finite and >= 0");
    if (c->H != h->H || c->Hp != h->Hp) return fail(h, FSMG_ERR_INVALID, "the cache's hidden size is not the handle's");
    int rc = check_group_ids(h, group, n, c->G);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    const Tiles tiles = make_tiles(n, c->G, [&](int q) { return group ? group[q] : 0; });
    AttendScratch as;
    if ((rc = attend_scratch(h, n, n_theta, tiles, true, &as)) != FSMG_OK) return rc;
    std::vector<float> qp((size_t)n * h->Hp, 0.0f);
    for (int q = 0; q < n; ++q) std::memcpy(qp.data() + (size_t)q * h->Hp, queries + (size_t)q * h->H, sizeof(float) * h->H);
    HIPCK(h, hipMemcpyAsync(as.Q, qp.data(), sizeof(float) * qp.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(as.tgt, targets, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if ((rc = attend_launch(h, c, tiles, as, n, as.Q, 0, as.tgt, thetas, n_theta)) != FSMG_OK) return rc;
    HIPCK(h, hipMemcpyAsync(out_prob, as.out, sizeof(float) * (size_t)n_theta * n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return FSMG_OK;
}

int fsmg_cache_distribution(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, int32_t n, const float* queries,
                            const float* logits, const int32_t* group, float* out_cache_prob, float* out_logprob, float* out_lse) {
    if (!h) return FSMG_ERR_INVALID;
    return distribution(h, cache, cc, nullptr, n, queries, logits, group, out_cache_prob, out_logprob, out_lse);
}

int fsmg_cache_self_distribution(fsmg_handle h, fsmg_cache cache, const fsmg_cache_gen_config* cc, const fsmg_cache_self_config* sc,
                                 int32_t n, const float* queries, const float* logits, const float* self_keys, const int32_t* self_values,
                                 const int32_t* self_len, int32_t S, const int32_t* group, float* out_cache_prob, float* out_logprob,
                                 float* out_lse) {
    if (!h) return FSMG_ERR_INVALID;
    const SelfEntries self{sc, self_keys, self_values, self_len, S};
    return distribution(h, cache, cc, &self, n, queries, logits, group, out_cache_prob, out_logprob, out_lse);
}

int fsmg_cache_score(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const int32_t* tokens, const int32_t* group,
                     float* out_logprob, float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* s = find_cache(h, cache);
    if (!s) return FSMG_ERR_INVALID;
    const void* outs[4] = {out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll};
    const int rc = check_score_config(h, s, c, tokens, group, outs);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, s, c, tokens, group, out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll);
}

int fsmg_cache_self_score(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const fsmg_cache_self_config* sc,
                          const int32_t* tokens, const int32_t* group, float* out_logprob, float* out_cache_prob,
                          float* out_lstm_logprob, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* s = nullptr;
    if (cache && !(s = find_cache(h, cache))) return FSMG_ERR_INVALID;
    fsmg_cache_s shape;                 // (no support cache: the checks read a shape, and the groups are ignored)
    shape.G = 1; shape.H = h->H; shape.Hp = h->Hp;
    if (!s) group = nullptr;
    const void* outs[4] = {out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll};
    int rc = check_score_config(h, s ? s : &shape, c, tokens, group, outs);
    if (rc == FSMG_OK) rc = check_self_config(h, sc);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, s, c, tokens, group, out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll, sc);
}

int fsmg_cache_self_attend(fsmg_handle h, fsmg_cache cache, const fsmg_cache_self_config* sc, int32_t n_rows, int32_t n_pos,
                           const float* vectors, const int32_t* values, const int32_t* group, const float* thetas, int32_t n_theta,
                           float* out_prob) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = nullptr;
    if (cache && !(c = find_cache(h, cache))) return FSMG_ERR_INVALID;
    int rc = check_self_config(h, sc);
    if (rc != FSMG_OK) return rc;
    if (n_rows < 1 || n_pos < 1 || (int64_t)n_rows * n_pos > (1 << 22)) return fail(h, FSMG_ERR_INVALID, "n_rows, n_pos must be >= 1 and n_rows * n_pos <= 2^22");
    if (!vectors || !values || !thetas || !out_prob) return fail(h, FSMG_ERR_INVALID, "null vectors / values / thetas / out_prob");
    if (n_theta < 1 || n_theta > FSMG_CACHE_MAX_THETA) return fail(h, FSMG_ERR_INVALID, "n_theta must be in [1, 8]");
    if (!thetas_ok(thetas, n_theta)) return fail(h, FSMG_ERR_INVALID, "every theta must be finite and >= 0");
    if (c && (c->H != h->H || c->Hp != h->Hp)) return fail(h, FSMG_ERR_INVALID, "the cache's hidden size is not the handle's");
    if (!c) group = nullptr;
    if (c && (rc = check_group_ids(h, group, n_rows, c->G)) != FSMG_OK) return rc;
    const int n = n_rows * n_pos;
    for (int i = 0; i < n; ++i)
        if (values[i] < 0 || values[i] >= h->V1) return fail(h, FSMG_ERR_TOKEN_RANGE, "value outside [0, input_size]");
    BEGIN_CALL(h);
    SelfScratch ss;
    if ((rc = self_scratch(h, n_rows, n, n_theta, true, &ss)) != FSMG_OK) return rc;
    const int Hp = h->Hp;
    std::vector<float> vp((size_t)n * Hp, 0.0f);
    for (int q = 0; q < n; ++q) std::memcpy(vp.data() + (size_t)q * Hp, vectors + (size_t)q * h->H, sizeof(float) * h->H);
    auto run = [&]() -> int {
        HIPCK(h, hipMemcpyAsync(ss.V, vp.data(), sizeof(float) * vp.size(), hipMemcpyHostToDevice, h->stream));
        HIPCK(h, hipMemcpyAsync(ss.val, values, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        const int r = self_launch(h, c, ss, n_rows, n_pos, sc->window, ss.V, (long long)n_pos * Hp, Hp, ss.val, n_pos, 1, group, thetas, n_theta);
        if (r != FSMG_OK) return r;
        HIPCK(h, hipMemcpyAsync(out_prob, ss.out, sizeof(float) * (size_t)n_theta * n, hipMemcpyDeviceToHost, h->stream));
        return FSMG_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(h->stream);       // the host vector goes out of scope
    if (rc == FSMG_OK && e != hipSuccess) return fail(h, FSMG_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}

// fsmg_cache_eval_step, and with `masked` fsmg_cache_eval_step_masked (support_len [N * K], query_len [N * Q] on the host)
static int cache_eval(fsmg_handle h, const int32_t* support, const int32_t* query, bool masked, const int32_t* support_len,
                      const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float theta, float lambda, float* nll) {
    if (!support || !query || !nll) return fail(h, FSMG_ERR_INVALID, "null support / query / nll");
    if (N < 1 || K < 1 || Q < 1 || (int64_t)N * K > (1 << 20) || (int64_t)N * Q > (1 << 20))
        return fail(h, FSMG_ERR_INVALID, "N, K, Q must be >= 1 and N * K, N * Q <= 2^20");
    fsmg_cache_config bc{};
    bc.version = FSMG_CACHE_CONFIG_VERSION; bc.n_rows = N * K; bc.n_groups = N;
    fsmg_cache_score_config sc{};
    sc.version = FSMG_CACHE_SCORE_CONFIG_VERSION; sc.n_rows = N * Q; sc.n_theta = 1; sc.n_lambda = 1;
    sc.thetas[0] = theta; sc.lambdas[0] = lambda;
    fsmg_cache_s shape;                 // the argument checks of both halves before any device work (check_score_config reads G and H)
    shape.G = N; shape.H = h->H; shape.Hp = h->Hp;
    fsmg_cache dummy = nullptr;
    std::vector<int32_t> group((size_t)N * Q);
    for (int r = 0; r < N * Q; ++r) group[r] = r / Q;
    std::vector<float> lp((size_t)N * Q * h->T);
    const void* outs[4] = {lp.data(), nullptr, nullptr, nullptr};
    int rc = check_build_config(h, &bc, support, &dummy);
    if (rc == FSMG_OK) rc = check_score_config(h, &shape, &sc, query, group.data(), outs);
    if (rc == FSMG_OK) rc = check_host_tokens(h, support, (size_t)N * K * h->T);
    if (rc == FSMG_OK) rc = check_host_tokens(h, query, (size_t)N * Q * h->T);
    if (rc == FSMG_OK && masked) rc = check_host_lengths(h, support_len, (size_t)N * K);
    if (rc == FSMG_OK && masked) rc = check_host_lengths(h, query_len, (size_t)N * Q);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    fsmg_cache_s* cache = nullptr;
    if ((rc = build_core(h, &bc, support, &cache, masked ? support_len : nullptr)) != FSMG_OK) return rc;
    rc = score_core(h, cache, &sc, query, group.data(), lp.data(), nullptr, nullptr, nullptr, nullptr, masked ? query_len : nullptr);
    hipStreamSynchronize(h->stream);
    free_cache(cache);                  // never registered: nobody else has seen it
    if (rc != FSMG_OK) return rc;
    double s = 0.0;
    if (!masked) {
        for (float v : lp) s += (double)v;
        *nll = (float)(-s / (double)lp.size());
        return FSMG_OK;
    }
    int64_t n_valid = 0;                // the scored positions in storage order
    for (int r = 0; r < N * Q; ++r) {
        for (int t = 0; t < query_len[r]; ++t) s += (double)lp[(size_t)r * h->T + t];
        n_valid += query_len[r];
    }
    *nll = (float)(-s / (double)n_valid);
    return FSMG_OK;
}

int fsmg_cache_eval_step(fsmg_handle h, const int32_t* support, const int32_t* query, int32_t N, int32_t K, int32_t Q, float theta,
                         float lambda, float* nll) {
    if (!h) return FSMG_ERR_INVALID;
    return cache_eval(h, support, query, false, nullptr, nullptr, N, K, Q, theta, lambda, nll);
}

int fsmg_cache_eval_step_masked(fsmg_handle h, const int32_t* support, const int32_t* query, const int32_t* support_len,
                                const int32_t* query_len, int32_t N, int32_t K, int32_t Q, float theta, float lambda, float* nll) {
    if (!h) return FSMG_ERR_INVALID;
    return cache_eval(h, support, query, true, support_len, query_len, N, K, Q, theta, lambda, nll);
}

int fsmg_cache_build_masked(fsmg_handle h, const fsmg_cache_config* c, const int32_t* tokens, const int32_t* lengths, fsmg_cache* out) {
    if (!h) return FSMG_ERR_INVALID;
    int rc = check_build_config(h, c, tokens, out);
    if (rc == FSMG_OK) rc = check_host_lengths(h, lengths, (size_t)c->n_rows);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    fsmg_cache_s* cache = nullptr;
    rc = build_core(h, c, tokens, &cache, lengths);
    if (rc != FSMG_OK) return rc;
    h->caches.push_back(cache);
    *out = cache;
    return FSMG_OK;
}

int fsmg_cache_create_from_counts(fsmg_handle h, int32_t n_groups, int32_t entries_per_group, const int32_t* counts, const float* keys,
                                  const int32_t* values, fsmg_cache* out) {
    if (!h) return FSMG_ERR_INVALID;
    if (!counts || !keys || !values || !out) return fail(h, FSMG_ERR_INVALID, "null counts / keys / values / out");
    int rc = check_cache_size(h, n_groups, entries_per_group);
    if (rc != FSMG_OK) return rc;
    const size_t G = (size_t)n_groups, Mg = (size_t)entries_per_group, n = G * Mg;
    for (size_t g = 0; g < G; ++g)
        if (counts[g] < 1 || counts[g] > entries_per_group) return fail(h, FSMG_ERR_INVALID, "every count must be in [1, entries_per_group]");
    for (size_t g = 0; g < G; ++g)      // the slots behind a count are not read
        for (size_t i = 0; i < (size_t)counts[g]; ++i)
            if (values[g * Mg + i] < 0 || values[g * Mg + i] >= h->V1) return fail(h, FSMG_ERR_TOKEN_RANGE, "cache value outside [0, input_size]");
    BEGIN_CALL(h);
    fsmg_cache_s* c = nullptr;
    if ((rc = alloc_cache(h, n_groups, entries_per_group, &c, true)) != FSMG_OK) return rc;
    c->n_g.assign(counts, counts + G);
    std::vector<float> kp(n * h->Hp, 0.0f);             // the pad units and the slots behind the counts are exact zeros
    std::vector<int> vp(n, 0);
    for (size_t g = 0; g < G; ++g)
        for (size_t i = 0; i < (size_t)counts[g]; ++i) {
            const size_t e = g * Mg + i;
            std::memcpy(kp.data() + e * h->Hp, keys + e * h->H, sizeof(float) * h->H);
            vp[e] = values[e];
        }
    hipError_t e = hipMemcpyAsync(c->keys, kp.data(), sizeof(float) * kp.size(), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->vals, vp.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->counts, c->n_g.data(), sizeof(int) * G, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);           // the host vectors go out of scope
    if (e != hipSuccess) { free_cache(c); return fail(h, FSMG_ERR_HIP, std::string("cache upload: ") + hipGetErrorString(e)); }
    h->caches.push_back(c);
    *out = c;
    return FSMG_OK;
}

int fsmg_cache_counts(fsmg_handle h, fsmg_cache cache, int32_t* out) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* c = find_cache(h, cache);
    if (!c) return FSMG_ERR_INVALID;
    if (!out) return fail(h, FSMG_ERR_INVALID, "null out");
    for (int g = 0; g < c->G; ++g) out[g] = c->entries(g);
    return FSMG_OK;
}

int fsmg_cache_score_masked(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const int32_t* tokens, const int32_t* lengths,
                            const int32_t* group, float* out_logprob, float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* s = find_cache(h, cache);
    if (!s) return FSMG_ERR_INVALID;
    const void* outs[4] = {out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll};
    int rc = check_score_config(h, s, c, tokens, group, outs);
    if (rc == FSMG_OK) rc = check_host_lengths(h, lengths, (size_t)c->n_rows);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, s, c, tokens, group, out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll, nullptr, lengths);
}

int fsmg_cache_self_score_masked(fsmg_handle h, fsmg_cache cache, const fsmg_cache_score_config* c, const fsmg_cache_self_config* sc,
                                 const int32_t* tokens, const int32_t* lengths, const int32_t* group, float* out_logprob,
                                 float* out_cache_prob, float* out_lstm_logprob, float* out_row_nll) {
    if (!h) return FSMG_ERR_INVALID;
    fsmg_cache_s* s = nullptr;
    if (cache && !(s = find_cache(h, cache))) return FSMG_ERR_INVALID;
    fsmg_cache_s shape;                 // (no support cache: the checks read a shape, and the groups are ignored)
    shape.G = 1; shape.H = h->H; shape.Hp = h->Hp;
    if (!s) group = nullptr;
    const void* outs[4] = {out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll};
    int rc = check_score_config(h, s ? s : &shape, c, tokens, group, outs);
    if (rc == FSMG_OK) rc = check_self_config(h, sc);
    if (rc == FSMG_OK) rc = check_host_lengths(h, lengths, (size_t)c->n_rows);
    if (rc != FSMG_OK) return rc;
    BEGIN_CALL(h);
    return score_core(h, s, c, tokens, group, out_logprob, out_cache_prob, out_lstm_logprob, out_row_nll, sc, lengths);
}

}  // extern "C"
