"""fp64 numpy restatement of fsmg_score's contract (include/fsmg.h "scoring of given songs") over a [rows, V1] logits array.

    logprob = z_y - lse,  lse = m + log(sum_v exp(z_v - m)),  m the row maximum
    rank    = #{v : z_v > z_y} + #{v < y : z_v == z_y}       (0-based, lower index first on ties)
    entropy = lse - sum_v p_v z_v,  p_v = exp(z_v - lse)       (a -inf column contributes 0)
    argmax  = the lowest index holding the row maximum
    row_nll = -(sum of logprob[t0:t1]) / (t1 - t0), fp64 in increasing t, rounded once to fp32

The fp64 logits of a model come from oracle.lstm_oracle.forward(...)[1]['logits'] (row b * T + t): oracle_logits()."""
import numpy as np

from oracle import lstm_oracle as O


def score_rows(z, y, dtype=np.float64):
    """z [rows, V1], y [rows] -> logprob, rank, entropy, argmax ([rows] each).  dtype = np.float32 evaluates the same formulas in
    fp32 (the CPU check of the GPU tests' tolerance)."""
    z = np.asarray(z, dtype)
    y = np.asarray(y).astype(np.int64)
    rows, V1 = z.shape
    r = np.arange(rows)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        m = z.max(axis=1)
        d = z - m[:, None]
        e = np.exp(d)
        S = e.sum(axis=1, dtype=dtype)
        lse = m + np.log(S)
        zy = z[r, y]
        logprob = zy - lse
        w = np.where(np.isneginf(d), dtype(0), e * d)           # p log p -> 0 at p = 0
        entropy = np.log(S) - w.sum(axis=1, dtype=dtype) / S
        cols = np.arange(V1)[None, :]
        rank = (z > zy[:, None]).sum(axis=1) + ((z == zy[:, None]) & (cols < y[:, None])).sum(axis=1)
    argmax = np.argmax(z, axis=1)                               # numpy: the first occurrence of the maximum
    return logprob, rank.astype(np.int64), entropy, argmax.astype(np.int64)


def row_nll(logprob, t0=0, count=0):
    """logprob [R, T] (any float dtype) -> float32 [R]: the fp64 sum in increasing t, rounded once"""
    lp = np.asarray(logprob)
    R, T = lp.shape
    t1 = t0 + count if count else T
    out = np.empty(R, np.float32)
    for r in range(R):
        s = 0.0
        for t in range(t0, t1):
            s += float(lp[r, t])
        out[r] = np.float32(-s / float(t1 - t0))
    return out


def oracle_logits(params64, songs, cfg):
    """fp64 logits [R * T, V1] (row b * T + t) and targets [R * T] of the songs [R, T] read as eval rows"""
    songs = np.asarray(songs).reshape(-1, cfg['max_len'])
    X, Y = O.eval_xy(songs[None], cfg['input_size'])
    _, cache = O.forward(params64, X, Y, cfg)
    return cache['logits'], Y.reshape(-1)


def score_songs(params64, songs, cfg):
    """-> dict of logprob / rank / entropy / argmax [R, T] and row_nll [R] in fp64 from the oracle's logits"""
    songs = np.asarray(songs).reshape(-1, cfg['max_len'])
    R, T = songs.shape
    z, y = oracle_logits(params64, songs, cfg)
    lp, rk, en, am = score_rows(z, y)
    return dict(logprob=lp.reshape(R, T), rank=rk.reshape(R, T), entropy=en.reshape(R, T), argmax=am.reshape(R, T),
                row_nll=-lp.reshape(R, T).mean(axis=1))


def rank_band(z64, y, eps=4e-5):
    """the ranks a computation whose logits are within eps / 2 of z64 may report: [#{z_v > z_y + eps}, #{v != y : z_v > z_y - eps}]"""
    z64 = np.asarray(z64, np.float64)
    y = np.asarray(y).astype(np.int64)
    r = np.arange(z64.shape[0])
    zy = z64[r, y][:, None]
    lo = (z64 > zy + eps).sum(axis=1)
    above = z64 > zy - eps
    above[r, y] = False
    return lo, above.sum(axis=1)


def known_bias(V1, seed=0):
    """A softmax_b for the known-answer tests: distinct values at least 0.01 apart (a shuffled 0.01 grid centred on 0), then two
    exactly equal pairs and one -inf entry.  -> (b float32 [V1], dict of the special columns).  With softmax_w = 0 the logits of
    every position are b exactly."""
    rng = np.random.RandomState(seed)
    b = ((rng.permutation(V1) - V1 // 2) * 0.01).astype(np.float32)
    V = V1 - 1                                                  # targets live in [0, V)
    cols = dict(pair_a=(3, V - 5), pair_b=(V // 2, V // 2 + 7), neg_inf=11)
    b[cols['pair_a'][1]] = b[cols['pair_a'][0]]
    b[cols['pair_b'][0]] = b[cols['pair_b'][1]]
    b[cols['neg_inf']] = -np.inf
    return b, cols


def known_songs(V1, R, T, cols, seed=0):
    """[R, T] targets that hit column 0, column input_size - 1, both members of both tied pairs and the -inf column"""
    V = V1 - 1
    songs = np.random.RandomState(seed + 1).randint(0, V, size=(R, T)).astype(np.int32)
    special = [0, V - 1, cols['neg_inf']] + list(cols['pair_a']) + list(cols['pair_b'])
    songs.reshape(-1)[:len(special)] = special
    songs[-1, -1] = V - 1
    return songs
