"""fp64 numpy restatement of per-song lengths in scoring and in the support-set cache (include/fsmg.h "per-song lengths in scoring
and in the support-set cache: ragged groups"), on top of tests/cache_ref.py:

    scored    position t of row r is scored iff t < len[r]
    entries   group g of the support rows holds, row-major and t increasing, the entries (row, t < len[row]) of cache_ref.entries:
              n_g = the sum of the group's lengths; the slots behind n_g, up to the capacity Mg = rows_per_group * T, are zeros
    attend    cache_ref.attend over the first n_g entries of the query's group
    outputs   cache_ref.score's at the scored positions, 0 behind a song's end; row_nll the mean over the scored positions of the
              window, NaN where there are none

A causal model's hidden state at t depends on the tokens before t alone, so the tokens at t >= len change nothing that is kept."""
import numpy as np

import cache_ref as R
import score_ref as S


def scored(lengths, T):
    """bool [R, T]"""
    return np.arange(T)[None, :] < np.asarray(lengths).reshape(-1)[:, None]


def entries(hidden, songs, n_groups, lengths):
    """hidden [R, T, H], songs [R, T], lengths [R] -> keys [G, Mg, H], values [G, Mg] (zeros behind the counts), counts [G]"""
    hidden, songs = np.asarray(hidden), np.asarray(songs)
    Rn, T, H = hidden.shape
    assert Rn % n_groups == 0
    rpg = Rn // n_groups
    keep = scored(lengths, T)
    keys = np.zeros((n_groups, rpg * T, H), hidden.dtype)
    vals = np.zeros((n_groups, rpg * T), songs.dtype)
    counts = np.zeros(n_groups, np.int32)
    for g in range(n_groups):
        rows = slice(g * rpg, (g + 1) * rpg)
        k = keep[rows].reshape(-1)
        n = int(k.sum())
        keys[g, :n] = hidden[rows].reshape(rpg * T, H)[k]
        vals[g, :n] = songs[rows].reshape(rpg * T)[k]
        counts[g] = n
    return keys, vals, counts


def attend_groups(keys, vals, counts, q, y, group, thetas, dtype=np.float64):
    """cache_ref.attend_groups over the first counts[g] entries of each group"""
    q = np.asarray(q)
    group = np.zeros(q.shape[0], np.int64) if group is None else np.asarray(group).astype(np.int64)
    out = np.zeros((len(thetas), q.shape[0]), dtype)
    for g in np.unique(group):
        sel = np.flatnonzero(group == g)
        n = int(counts[g])
        out[:, sel] = R.attend(keys[g][:n], vals[g][:n], q[sel], np.asarray(y)[sel], thetas, dtype)
    return out


def row_nll(logprob, lengths, nll_first=0, nll_count=0):
    """logprob [.., R, T] -> float32 [.., R]: -(fp64 sum in increasing t over the scored positions of the window) / their number,
    rounded once; NaN for an empty window (the library's loop, so that the bits can be compared)"""
    lp = np.asarray(logprob)
    T = lp.shape[-1]
    t1 = nll_first + nll_count if nll_count else T
    flat = lp.reshape(-1, lp.shape[-2], T)
    out = np.empty(flat.shape[:2], np.float32)
    for p in range(flat.shape[0]):
        for r in range(flat.shape[1]):
            te = min(t1, int(np.asarray(lengths).reshape(-1)[r]))
            s = 0.0
            for t in range(nll_first, te):
                s += float(flat[p, r, t])
            out[p, r] = np.float32(-s / (te - nll_first)) if te > nll_first else np.float32(np.nan)
    return out.reshape(lp.shape[:-1])


def oracle_pass(params64, support, query, cfg):
    """what every length setting of one (support, query) pair shares: the fp64 hidden states, targets and model log-probs"""
    support = np.asarray(support).reshape(-1, cfg['max_len'])
    query = np.asarray(query).reshape(-1, cfg['max_len'])
    hs, _ = R.oracle_hidden(params64, support, cfg)
    hq, y = R.oracle_hidden(params64, query, cfg)
    z, yy = S.oracle_logits(params64, query, cfg)
    lp = S.score_rows(z, yy)[0].reshape(query.shape)
    return dict(support=support, query=query, hs=hs, hq=hq, y=y, lp=lp)


def score(oracle, n_groups, support_len, query_len, group, thetas, lambdas, nll_first=0, nll_count=0):
    """fsmg_cache_build_masked + fsmg_cache_score_masked in fp64 from oracle_pass's dict: lstm_logprob [R, T], cache_prob [k, R, T],
    logprob [k, j, R, T] (fp64, 0 behind a song's end), row_nll [k, j, R] (fp64 means over the scored positions of the window, NaN
    for none), and keys / values / counts / queries / scored"""
    query = oracle['query']
    Rn, T = query.shape
    keys, vals, counts = entries(oracle['hs'], oracle['support'], n_groups, support_len)
    keep = scored(query_len, T)
    grp = np.zeros(Rn, np.int64) if group is None else np.asarray(group)
    pc = attend_groups(keys, vals, counts, oracle['hq'].reshape(Rn * T, -1), oracle['y'].reshape(-1), np.repeat(grp, T),
                       thetas).reshape(len(thetas), Rn, T)
    lp = np.where(keep, oracle['lp'], 0.0)
    pc = np.where(keep[None], pc, 0.0)
    out = np.zeros((len(thetas), len(lambdas), Rn, T))
    for k in range(len(thetas)):
        for j, lam in enumerate(lambdas):
            out[k, j] = np.where(keep, R.mix64(oracle['lp'], pc[k], lam), 0.0)
    t1 = nll_first + nll_count if nll_count else T
    win = keep[:, nll_first:t1]           # (the window's slice, so that full lengths sum what cache_ref's mean sums)
    with np.errstate(invalid='ignore', divide='ignore'):
        nll = -np.where(win, out[..., nll_first:t1], 0.0).sum(axis=-1) / win.sum(axis=-1)
    return dict(lstm_logprob=lp, cache_prob=pc, logprob=out, row_nll=nll, keys=keys, values=vals, counts=counts,
                queries=oracle['hq'], scored=keep)
