"""fp64 numpy restatement of the support-set cache's contract (include/fsmg.h "support-set neural cache").

    entries   row r of the support rows [n_rows, T] belongs to group r // (n_rows // G); entry (r % rows_per_group) * T + t of the
              group: key = the top-layer h after the inputs [start, x_0 .. x_{t-1}], value = x_t
    attend    d_i = q . k_i over the group's keys;  p_cache(y) = sum_{i : v_i = y} exp(theta (d_i - d_max)) / sum_i exp(theta (d_i - d_max))
    mix       log((1 - lambda) exp(lp) + lambda p_cache) = logaddexp(log1p(-lambda) + lp, log(lambda) + log(p_cache)), in fp64,
              rounded once to fp32
    row_nll   score_ref.row_nll over the mixed log-probs

The fp64 hidden states of a model come from oracle.lstm_oracle.forward(...)[1]['out'] (row b * T + t): oracle_hidden().
dtype = np.float32 evaluates attend's formulas in fp32 (the GPU tests' tolerance is derived from its error)."""
import numpy as np

import score_ref as S
from oracle import lstm_oracle as O


def attend(keys, vals, q, y, thetas, dtype=np.float64):
    """one group: keys [Mg, H], vals [Mg], q [n, H], y [n], thetas [k] -> p_cache [k, n] in dtype"""
    keys, q = np.asarray(keys, dtype), np.asarray(q, dtype)
    vals, y = np.asarray(vals).astype(np.int64), np.asarray(y).astype(np.int64)
    d = q.dot(keys.T)                                            # [n, Mg]
    x = d - d.max(axis=1, keepdims=True)
    hit = vals[None, :] == y[:, None]
    out = np.empty((len(thetas), q.shape[0]), dtype)
    for k, th in enumerate(thetas):
        e = np.exp(dtype(th) * x)
        out[k] = np.where(hit, e, dtype(0)).sum(axis=1, dtype=dtype) / e.sum(axis=1, dtype=dtype)
    return out


def attend_groups(keys, vals, q, y, group, thetas, dtype=np.float64):
    """keys [G, Mg, H], vals [G, Mg], q [n, H], y [n], group [n] (None: all 0) -> p_cache [k, n] in dtype"""
    q = np.asarray(q)
    group = np.zeros(q.shape[0], np.int64) if group is None else np.asarray(group).astype(np.int64)
    out = np.zeros((len(thetas), q.shape[0]), dtype)
    for g in np.unique(group):
        sel = np.flatnonzero(group == g)
        out[:, sel] = attend(keys[g], vals[g], q[sel], np.asarray(y)[sel], thetas, dtype)
    return out


def mix(lp, pc, lam):
    """lp, pc arrays of one shape (any float dtype), lam a scalar in [0, 1] -> float32: the fp64 mixture, rounded once"""
    lp, pc = np.asarray(lp, np.float64), np.asarray(pc, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        a = np.log1p(-np.float64(lam)) + lp
        b = np.log(np.float64(lam)) + np.log(pc)
        return np.logaddexp(a, b).astype(np.float32)


def mix64(lp, pc, lam):
    """the same in fp64, not rounded"""
    lp, pc = np.asarray(lp, np.float64), np.asarray(pc, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.logaddexp(np.log1p(-np.float64(lam)) + lp, np.log(np.float64(lam)) + np.log(pc))


def oracle_hidden(params64, songs, cfg):
    """fp64 top-layer hidden states [R, T, H] and targets [R, T] of the songs [R, T] read as eval rows"""
    songs = np.asarray(songs).reshape(-1, cfg['max_len'])
    R, T = songs.shape
    X, Y = O.eval_xy(songs[None], cfg['input_size'])
    _, cache = O.forward(params64, X, Y, cfg)
    return cache['out'].reshape(R, T, -1), Y.reshape(R, T)


def entries(hidden, songs, n_groups):
    """hidden [R, T, H], songs [R, T] -> keys [G, Mg, H], values [G, Mg], Mg = (R // G) * T"""
    R, T, H = hidden.shape
    assert R % n_groups == 0
    return hidden.reshape(n_groups, R // n_groups * T, H), np.asarray(songs).reshape(n_groups, R // n_groups * T)


def score(params64, support, n_groups, query, group, thetas, lambdas, cfg, nll_first=0, nll_count=0):
    """fsmg_cache_build + fsmg_cache_score in fp64 from the oracle: a dict of lstm_logprob [R, T], cache_prob [k, R, T], logprob
    [k, j, R, T] (fp64, not rounded), row_nll [k, j, R], and the vectors: keys, values, queries [R, T, H]"""
    support = np.asarray(support).reshape(-1, cfg['max_len'])
    query = np.asarray(query).reshape(-1, cfg['max_len'])
    R, T = query.shape
    hs, _ = oracle_hidden(params64, support, cfg)
    keys, vals = entries(hs, support, n_groups)
    hq, y = oracle_hidden(params64, query, cfg)
    z, yy = S.oracle_logits(params64, query, cfg)
    lp = S.score_rows(z, yy)[0].reshape(R, T)
    grp = np.zeros(R, np.int64) if group is None else np.asarray(group)
    pc = attend_groups(keys, vals, hq.reshape(R * T, -1), y.reshape(-1), np.repeat(grp, T), thetas).reshape(len(thetas), R, T)
    out = np.empty((len(thetas), len(lambdas), R, T))
    for k in range(len(thetas)):
        for j, lam in enumerate(lambdas):
            out[k, j] = mix64(lp, pc[k], lam)
    t1 = nll_first + nll_count if nll_count else T
    return dict(lstm_logprob=lp, cache_prob=pc, logprob=out, row_nll=-out[..., nll_first:t1].mean(axis=-1), keys=keys, values=vals,
                queries=hq)
