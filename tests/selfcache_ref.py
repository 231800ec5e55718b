"""fp64 numpy restatement of the self-cache's contract (include/fsmg.h "self-cache"), on top of cache_ref.py.

    own entries   own entry i of a row is (key = q_i, value = x_i): q_i the top-layer h after input i of [start, x_0 .. x_{T-2}]
    window        position t sees its own entries max(0, t - W) .. t - 1 (never entry t, whose value is the target)
    union         with support entries (keys [Mg, H], vals [Mg] of the row's group) one softmax over both:
                  p_cache(y) = sum_{i in set, v_i = y} exp(theta (d_i - d_max)) / sum_{i in set} exp(theta (d_i - d_max)),  d_i = q_t . k_i
    empty set     no support entries and t = 0: p_cache = 0 and the mixed log-prob is the model's lp at every lambda

attend() is the masked-matrix form; explicit_entries() spells a position's set out as a list, for cache_ref.attend.
dtype = np.float32 evaluates attend's formulas in fp32 (the GPU tests' tolerance is derived from its error)."""
import numpy as np

import cache_ref as R
import score_ref as S


def visible(T, W, Mg=0):
    """bool [T, Mg + T]: column j < Mg is support entry j (always visible), column Mg + i is own entry i (t - W <= i < t)"""
    t = np.arange(T)[:, None]
    i = np.arange(T)[None, :]
    own = (i < t) & (i >= t - int(W))
    return np.concatenate([np.ones((T, Mg), bool), own], axis=1)


def attend(vec, val, W, thetas, keys=None, vals=None, dtype=np.float64):
    """one row: vec [T, H] (query t and own key t), val [T] (target t and own value t), support keys [Mg, H] / vals [Mg] or None
    -> p_cache [k, T] in dtype; exactly 0 where the visible set is empty or holds no val[t]"""
    vec = np.asarray(vec, dtype)
    val = np.asarray(val).astype(np.int64)
    T, H = vec.shape
    keys = np.zeros((0, H), dtype) if keys is None else np.asarray(keys, dtype)
    vals = np.zeros(0, np.int64) if vals is None else np.asarray(vals).astype(np.int64)
    K = np.concatenate([keys, vec], axis=0)                     # [Mg + T, H]
    V = np.concatenate([vals, val])
    see = visible(T, W, keys.shape[0])
    d = vec.dot(K.T)                                            # [T, Mg + T]
    neg = dtype(-np.inf)
    dm = np.where(see, d, neg).max(axis=1, keepdims=True)
    some = see.any(axis=1)
    dm = np.where(some[:, None], dm, dtype(0))                  # (an empty row: no entry, nothing to shift)
    hit = see & (V[None, :] == val[:, None])
    out = np.zeros((len(thetas), T), dtype)
    for k, th in enumerate(thetas):
        with np.errstate(over='ignore', invalid='ignore'):
            e = np.where(see, np.exp(dtype(th) * (d - dm)), dtype(0))
        den = e.sum(axis=1, dtype=dtype)
        num = np.where(hit, e, dtype(0)).sum(axis=1, dtype=dtype)
        out[k] = np.where(some, num / np.where(some, den, dtype(1)), dtype(0))
    return out


def attend_rows(vec, val, W, thetas, keys=None, vals=None, group=None, dtype=np.float64):
    """vec [R, T, H], val [R, T]; support keys [G, Mg, H], vals [G, Mg] or None; group [R] (None: all 0) -> [k, R, T]"""
    vec = np.asarray(vec)
    n = vec.shape[0]
    group = np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64)
    out = np.zeros((len(thetas), n, vec.shape[1]), dtype)
    for r in range(n):
        kg, vg = (None, None) if keys is None else (keys[group[r]], vals[group[r]])
        out[:, r] = attend(vec[r], val[r], W, thetas, kg, vg, dtype)
    return out


def explicit_entries(vec, val, t, W, keys=None, vals=None):
    """the set of position t as a list: [support entries ++ own entries max(0, t - W) .. t - 1] -> keys [n, H], vals [n]"""
    vec, val = np.asarray(vec), np.asarray(val)
    lo = max(0, t - int(W))
    k, v = vec[lo:t], val[lo:t]
    if keys is not None:
        k, v = np.concatenate([np.asarray(keys, vec.dtype), k], axis=0), np.concatenate([np.asarray(vals), v])
    return k, v


def mix64(lp, pc, lam, empty):
    """cache_ref.mix64 with the empty-set rule: where `empty` (bool, broadcast against lp) the model's lp at every lambda"""
    lp = np.asarray(lp, np.float64)
    return np.where(empty, lp, R.mix64(lp, pc, lam))


def mix(lp, pc, lam, empty):
    """cache_ref.mix (fp32, rounded once) with the empty-set rule; lp bitwise where `empty`"""
    return np.where(empty, np.asarray(lp, np.float32), R.mix(lp, pc, lam))


def empty_positions(T, with_support):
    """bool [T]: the positions whose set is empty"""
    e = np.zeros(T, bool)
    e[0] = not with_support
    return e


def score(params64, query, W, thetas, lambdas, cfg, support=None, n_groups=1, group=None, nll_first=0, nll_count=0):
    """fsmg_cache_self_score in fp64 from the oracle (support None: the pure self-cache): a dict of lstm_logprob [R, T], cache_prob
    [k, R, T], logprob [k, j, R, T] (fp64, not rounded), row_nll [k, j, R], and the vectors: queries [R, T, H], keys, values"""
    query = np.asarray(query).reshape(-1, cfg['max_len'])
    n, T = query.shape
    keys = vals = None
    if support is not None:
        support = np.asarray(support).reshape(-1, cfg['max_len'])
        hs, _ = R.oracle_hidden(params64, support, cfg)
        keys, vals = R.entries(hs, support, n_groups)
    hq, y = R.oracle_hidden(params64, query, cfg)
    z, yy = S.oracle_logits(params64, query, cfg)
    lp = S.score_rows(z, yy)[0].reshape(n, T)
    pc = attend_rows(hq, y, W, thetas, keys, vals, group)
    empty = empty_positions(T, support is not None)[None, :]
    out = np.empty((len(thetas), len(lambdas), n, T))
    for k in range(len(thetas)):
        for j, lam in enumerate(lambdas):
            out[k, j] = mix64(lp, pc[k], lam, empty)
    t1 = nll_first + nll_count if nll_count else T
    return dict(lstm_logprob=lp, cache_prob=pc, logprob=out, row_nll=-out[..., nll_first:t1].mean(axis=-1), keys=keys, values=vals,
                queries=hq)


def copied_half_song(cfg, seed=5):
    """a song [T] whose second half copies its first half"""
    T = cfg['max_len']
    half = np.random.RandomState(seed).randint(0, cfg['input_size'], size=(T + 1) // 2)
    return np.concatenate([half, half])[:T].astype(np.int32)


def copied_half_gain(lp_mix, lp_lstm):
    """per-token gain (nats) of the mixture over the model alone on one row: mean(lp_mix) - mean(lp_lstm), in fp64"""
    return float(np.asarray(lp_mix, np.float64).mean() - np.asarray(lp_lstm, np.float64).mean())


# ------------------------------------------------------------------------------------------------ the oracle tests' inputs
GROUP = np.array([0, 0, 1, 1, 0], np.int32)         # 5 query rows over the 2 support groups
LAMBDAS = [0.0, 0.25, 1.0]
GAIN_LAMBDA = 0.25
DEFAULT_THETA = 1.0                                  # config/cache_lstm.yaml's cache_theta
TUNE_THETAS = [0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0]


def oracle_case(name):
    """cachegen_ref.oracle_case(name) (the oracle's parameters after three of its train steps, as a handle holds them; 6 support rows
    in 2 groups) plus: query [5, T], row 0 the copied-half song; thetas: theta * dmax = 0.3, 5, 40 with dmax the largest |q . k| of the
    fp64 vectors over the union's pairs at W = T"""
    import cachegen_ref as CG
    case = dict(CG.oracle_case(name))
    cfg = case['cfg']
    query = np.random.RandomState(12).randint(0, cfg['input_size'], size=(5, cfg['max_len'])).astype(np.int32)
    query[0] = copied_half_song(cfg)
    hq, _ = R.oracle_hidden(case['params'], query, cfg)
    k64 = case['keys'].astype(np.float64)
    dmax = max(max(float(np.abs(hq[r].dot(k64[GROUP[r]].T)).max()), float(np.abs(hq[r].dot(hq[r].T)).max())) for r in range(5))
    case.update(query=query, group=GROUP, thetas=[float(np.float32(x / dmax)) for x in (0.3, 5.0, 40.0)], dmax=dmax)
    return case


def gain_theta(case):
    """the theta of the copied-half leg: the default where the fp64 mixture gains over the model alone at GAIN_LAMBDA on the
    copied-half song (pure self-cache, W = T), else the best of tune's grid -> (theta, fp64 gain, whether the default was kept)"""
    cfg = case['cfg']
    T = cfg['max_len']
    ref = score(case['params'], case['query'][:1], T, [DEFAULT_THETA] + TUNE_THETAS, [GAIN_LAMBDA], cfg)
    gains = [copied_half_gain(ref['logprob'][k, 0, 0], ref['lstm_logprob'][0]) for k in range(1 + len(TUNE_THETAS))]
    if gains[0] > 0:
        return DEFAULT_THETA, gains[0], True
    k = int(np.argmax(gains[1:]))
    return TUNE_THETAS[k], gains[1 + k], False


# ------------------------------------------------------------------------------------------------ decode time
def union_entries(own_keys, own_vals, n_own, W, keys_g=None, vals_g=None):
    """[support entries ++ the last min(n_own, W) of the first n_own own entries] -> keys [n, H], vals [n] (n may be 0)"""
    own_keys, own_vals = np.asarray(own_keys), np.asarray(own_vals)
    n = min(int(n_own), int(W))
    k, v = own_keys[n_own - n:n_own], own_vals[n_own - n:n_own]
    if keys_g is not None:
        k = np.concatenate([np.asarray(keys_g, k.dtype if k.size else np.asarray(keys_g).dtype).reshape(-1, own_keys.shape[-1]), k], axis=0)
        v = np.concatenate([np.asarray(vals_g), v])
    return k, v.astype(np.int64)


def distribution(q, z, self_keys, self_vals, self_len, W, theta, lam, keys=None, vals=None, group=None, dtype=np.float64):
    """fsmg_cache_self_distribution: q [n, H], logits z [n, V1], self_keys [n, S, H], self_vals [n, S], self_len [n]; support keys [G, Mg,
    H] / vals [G, Mg] or None -> dict: cache_prob [n, V1] in dtype, lse [n], lp [n, V1], logprob [n, V1] (z'', fp64, not rounded); an
    empty union gives cache_prob 0 and logprob = lp"""
    import cachegen_ref as CG
    import gen_ref as G
    z = np.asarray(z, np.float64)
    n, V1 = z.shape
    group = np.zeros(n, np.int64) if group is None else np.asarray(group).astype(np.int64)
    pc = np.zeros((n, V1), dtype)
    lse = np.array([G.logsumexp(row) for row in z])
    lp = z - lse[:, None]
    out = np.empty((n, V1))
    for i in range(n):
        kg, vg = (None, None) if keys is None else (keys[group[i]], vals[group[i]])
        k, v = union_entries(self_keys[i], self_vals[i], self_len[i], W, kg, vg)
        if len(v) == 0:
            out[i] = lp[i]
            continue
        pc[i] = CG.cache_prob(k, v, np.asarray(q)[i][None], theta, V1, dtype)[0]
        out[i] = R.mix64(lp[i], pc[i], lam)
    return dict(cache_prob=pc, lse=lse, lp=lp, logprob=out)


def _visible_tol(theta, q, k):
    """cachegen_ref.tolerance over the entries the position sees (none: the model's own 1e-4)"""
    import cachegen_ref as CG
    return CG.tolerance(theta, CG.l1_of(q, k)) if len(k) else CG.tolerance(0.0, 0.0)


def _decode_row(params, config, inputs, W, theta, lam, keys_g, vals_g):
    """one row teacher-forced over `inputs` (own entry j: the top-layer h after input j, value inputs[j + 1]) -> z'' [len, V1] and the
    tolerance of each position"""
    import gen_ref as G
    from oracle import lstm_oracle as O
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    hs = [np.zeros(H) for _ in range(L)]
    cs = [np.zeros(H) for _ in range(L)]
    own, rows, tols = [], [], []
    for p, w in enumerate(inputs):
        lg = G._cell_step(params, H, L, params['embedding'][w], hs, cs)
        q = hs[L - 1].copy()
        k, v = union_entries(np.array(own).reshape(-1, H), np.asarray(inputs[1:p + 1], np.int64), p, W, keys_g, vals_g)
        lp = lg - G.logsumexp(lg)
        if len(v) == 0:
            rows.append(lp)
        else:
            import cachegen_ref as CG
            rows.append(R.mix64(lp, CG.cache_prob(k, v, q[None], theta, d['V1'])[0], lam))
        tols.append(_visible_tol(theta, q, k))
        own.append(q)
    return np.stack(rows), np.array(tols)


def generate(params, config, W, theta, lam, n_seq, num, keys=None, vals=None, group=None, temperature=1.0, top_k=0, seed=0, primer=None):
    """the free-running fp64 draw from the union's mixture (cachegen_ref.generate with the own-history step) -> dict: toks [B, num],
    lps, margin (the fp64 margin of each pick), tol (the tolerance of each position)"""
    import cachegen_ref as CG
    import gen_ref as G
    from oracle import lstm_oracle as O
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    P = 0 if primer is None else np.asarray(primer).shape[1]
    group = np.zeros(n_seq, np.int64) if group is None else np.asarray(group)
    out = dict(toks=np.zeros((n_seq, num), np.int64), lps=np.zeros((n_seq, num)), margin=np.zeros((n_seq, num)), tol=np.zeros((n_seq, num)))
    for b in range(n_seq):
        kg, vg = (None, None) if keys is None else (np.asarray(keys[group[b]], np.float64), vals[group[b]])
        hs = [np.zeros(H) for _ in range(L)]
        cs = [np.zeros(H) for _ in range(L)]
        buf = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]])
        own = []
        for p in range(P + num):
            lg = G._cell_step(params, H, L, params['embedding'][buf[p]], hs, cs)
            q = hs[L - 1].copy()
            if p >= P:
                k, v = union_entries(np.array(own).reshape(-1, H), np.asarray(buf[1:p + 1], np.int64), p, W, kg, vg)
                lp = lg - G.logsumexp(lg)
                zz = lp if len(v) == 0 else R.mix64(lp, CG.cache_prob(k, v, q[None], theta, d['V1'])[0], lam)
                t = p - P
                w, score = G.choose(zz, temperature, top_k, G.gumbel(seed, t, b, d['V1']))
                out['toks'][b, t], out['lps'][b, t] = w, zz[w] - G.logsumexp(zz)
                out['margin'][b, t], out['tol'][b, t] = CG._margin(score), _visible_tol(theta, q, k)
                buf.append(int(w))
            own.append(q)
    return out


def check_margins(params, config, W, theta, lam, toks, lps, temperature, top_k, seed, keys=None, vals=None, group=None, primer=None,
                  tokens=True):
    """cachegen_ref.check_margins on the union's rows: row b's own token history is fed into the fp64 decoder; at every generated
    position the GPU log-prob is within the position's tolerance of the fp64 one, the GPU token's perturbed score within it of the
    fp64 maximum, and the token the fp64 choice wherever the fp64 margin is >= twice the tolerance
    -> dict: near, total, lp_err, lp_tol, slack, tol_min, tol_max"""
    import cachegen_ref as CG
    import gen_ref as G
    from oracle import lstm_oracle as O
    d = O.model_dims(config)
    B, num = toks.shape
    P = 0 if primer is None else np.asarray(primer).shape[1]
    group = np.zeros(B, np.int64) if group is None else np.asarray(group)
    res = dict(near=0, total=0, lp_err=0.0, lp_tol=0.0, slack=0.0, tol_min=np.inf, tol_max=0.0)
    for b in range(B):
        kg, vg = (None, None) if keys is None else (np.asarray(keys[group[b]], np.float64), vals[group[b]])
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[b]]) + [int(w) for w in toks[b]]
        zz_all, tol_all = _decode_row(params, config, inputs[:-1] + [inputs[-1]], W, theta, lam, kg, vg)
        for t in range(num):
            zz, tol, g = zz_all[P + t], float(tol_all[P + t]), int(toks[b, t])
            assert 0 <= g < d['V1'], (b, t, g)
            res['total'] += 1
            res['tol_min'], res['tol_max'] = min(res['tol_min'], tol), max(res['tol_max'], tol)
            want_lp = zz[g] - G.logsumexp(zz)
            assert np.isfinite(want_lp), ('a token the fp64 mixture gives no mass', b, t, g)
            e = abs(float(lps[b, t]) - want_lp)
            if e > res['lp_err']:
                res['lp_err'], res['lp_tol'] = e, tol
            assert e <= tol, ('logprob', b, t, lps[b, t], want_lp, tol)
            if not tokens:
                continue
            noise = G.gumbel(seed, t, b, d['V1'])
            want, score = G.choose(zz, temperature, top_k, noise)
            sg = zz[g] if temperature == 0 or top_k == 1 else zz[g] / temperature + noise[g]
            res['slack'] = max(res['slack'], float(score[want] - sg))
            assert sg >= score[want] - tol, ('margin', b, t, g, want, sg, score[want], tol)
            if CG._margin(score) >= 2 * tol:
                assert g == want, ('token', b, t, g, want, CG._margin(score), tol)
            else:
                res['near'] += 1
    return res


GEN_NUM, GEN_W, GEN_SEED = 12, 6, 21
GEN_PICKS = ((1.0, 0), (0.7, 5))                    # (temperature, top_k)
