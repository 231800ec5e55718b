"""numpy restatement of fsmg_beam_search (include/fsmg.h, DESIGN.md "Beam search"), built on the fp64 decoder of gen_ref, and the
checks the GPU tests use.  A candidate (slot j, column v) has lp = logit_v - lse_j and score s = cum_j + lp; a group's candidates
rank by s descending, then j ascending, then logit descending, then v ascending, a NaN s or logit below -inf."""
import itertools

import numpy as np

import gen_ref as R
from oracle import lstm_oracle as O


def lse_of(logits, dtype=np.float64):
    """the row's logsumexp: max + log(sum exp(logit - max)) (the device sums in double)"""
    lg = np.asarray(logits, np.float64)
    mx = np.max(lg)
    return dtype(mx + np.log(np.sum(np.exp(lg - mx))))


def rank(cum, logits, dtype=np.float64, lse=None):
    """one step of one group: cum [W'], logits [W', V1] -> (order, s, lp), order = the (j, v) pairs of every candidate best
    first, s / lp [W', V1] (in dtype: float32 restates the device's rounding of lp and s)"""
    cum = np.asarray(cum, dtype)
    lg = np.asarray(logits, dtype)
    Wn, V1 = lg.shape
    if lse is None:
        lse = np.array([lse_of(lg[j], dtype) for j in range(Wn)], dtype)
    with np.errstate(invalid='ignore'):
        lp = (lg - np.asarray(lse, dtype)[:, None]).astype(dtype)
        s = (cum[:, None] + lp).astype(dtype)
    j = np.repeat(np.arange(Wn), V1)
    v = np.tile(np.arange(V1), Wn)
    sf, lf = s.ravel(), lg.ravel()
    s_nan, l_nan = np.isnan(sf), np.isnan(lf)
    s_key = np.where(s_nan, 0.0, -sf.astype(np.float64))
    l_key = np.where(l_nan, 0.0, -lf.astype(np.float64))
    # np.lexsort: the last key is the primary one, each ascending; -0.0 and 0.0 compare equal
    idx = np.lexsort((v, l_key, l_nan, j, s_key, s_nan))
    return [(int(j[i]), int(v[i])) for i in idx], s, lp


def _gaps(order, s, W):
    """the smallest difference between adjacent ranks among the first W + 1 candidates with a finite score"""
    vals = [float(s[j, v]) for j, v in order[:W + 1]]
    vals = [x for x in vals if np.isfinite(x)]
    if len(vals) < 2:
        return np.inf
    return float(np.min(np.abs(np.diff(vals))))


def _new_state(d):
    return [np.zeros(d['H']) for _ in range(d['L'])], [np.zeros(d['H']) for _ in range(d['L'])]


def beam_search(params, config, n_groups, W, num, primer=None):
    """the fp64 beam search -> tokens int [G, W, num], scores [G, W], lps [G, W, num], gaps [G, num] (per generated position, the
    smallest score gap between adjacent ranks among the W + 1 best finite candidates: the W / W+1 boundary included)"""
    d = O.model_dims(config)
    H, L, V1 = d['H'], d['L'], d['V1']
    P = 0 if primer is None else np.asarray(primer).shape[1]
    toks = np.zeros((n_groups, W, num), np.int64)
    lps = np.zeros((n_groups, W, num))
    scores = np.zeros((n_groups, W))
    gaps = np.zeros((n_groups, num))
    for g in range(n_groups):
        hs, cs = _new_state(d)
        inputs = [d['start']] + ([] if P == 0 else [int(w) for w in primer[g]])
        for w in inputs[:-1]:
            R._cell_step(params, H, L, params['embedding'][w], hs, cs)
        # every slot starts from the group's state; slot 0 is the only live one
        slots = [([h.copy() for h in hs], [c.copy() for c in cs], inputs[-1], [], []) for _ in range(W)]
        cum = np.array([0.0] + [-np.inf] * (W - 1))
        for t in range(num):
            logits = np.stack([R._cell_step(params, H, L, params['embedding'][w], sh, sc) for sh, sc, w, _, _ in slots])
            order, s, lp = rank(cum, logits)
            gaps[g, t] = _gaps(order, s, W)
            new = []
            for j, v in order[:W]:
                sh, sc, _, tk, lk = slots[j]
                new.append(([h.copy() for h in sh], [c.copy() for c in sc], v, tk + [v], lk + [float(lp[j, v])]))
            cum = np.array([s[j, v] for j, v in order[:W]])
            slots = new
        for n in range(W):
            toks[g, n] = slots[n][3]
            lps[g, n] = slots[n][4]
        scores[g] = cum
    return toks, scores, lps, gaps


def sequence_logprobs(params, config, seq, primer_row=None):
    """teacher-forced fp64 log-probs of one continuation seq (after [start, primer_row])"""
    d = O.model_dims(config)
    pre = [d['start']] + ([] if primer_row is None else [int(w) for w in primer_row])
    lg = R.row_logits(params, config, pre + [int(w) for w in seq[:-1]])[len(pre) - 1:]
    return np.array([lg[t, int(seq[t])] - R.logsumexp(lg[t]) for t in range(len(seq))])


def enumerate_all(params, config, num, primer_row=None):
    """every V1^num continuation and its fp64 log-likelihood, best first (ties by sequence) -> (seqs [n, num], scores [n])"""
    d = O.model_dims(config)
    seqs = np.array(list(itertools.product(range(d['V1']), repeat=num)), np.int64)
    sc = np.array([sequence_logprobs(params, config, q, primer_row).sum() for q in seqs])
    order = np.lexsort(tuple(seqs[:, k] for k in range(num - 1, -1, -1)) + (-sc,))
    return seqs[order], sc[order]


def fp32_sum(lps):
    """the fp32 left-to-right sum the device's score is, bitwise"""
    s = np.float32(0.0)
    for x in np.asarray(lps, np.float32):
        s = np.float32(s + x)
    return s
