"""numpy restatement of fsmg_generate_filtered (include/fsmg.h, DESIGN.md "Sampling filters"): the repetition penalty, the top-k,
min-p and top-p sets in fp64, the draw over them (gen_ref's Philox / Gumbel), the free-running fp64 decoder, and the teacher-forced
margin check the GPU tests use."""
import numpy as np

import gen_ref as R
from oracle import lstm_oracle as O

BOUNDARY = 1e-5     # a column's in / out decision may differ from fp64 only this close to a min-p or top-p boundary


def neutral(top_p=0.0, min_p=0.0, theta=1.0):
    return top_p in (0.0, 1.0) and min_p == 0.0 and theta in (0.0, 1.0)


def penalise(z, context, theta, window):
    """step 1: z' = z with the distinct ids of the last `window` context tokens (0: all of them) penalised once each"""
    zp = np.array(z, np.float64)
    if theta in (0.0, 1.0):
        return zp
    ctx = [int(w) for w in context]
    if window > 0:
        ctx = ctx[-window:] if ctx else []
    for v in set(ctx):
        zp[v] = zp[v] / theta if zp[v] > 0 else zp[v] * theta
    return zp


def filter_sets(zp, temperature, top_k, top_p, min_p):
    """steps 2-4 at T > 0 -> dict: A (top-k set), S (after min-p), F (final set), d = (z' - z'max) / T (0 at z'max),
    ahead (top-p mass of the survivors with strictly larger z', 0 outside S), thr_k (the top-k threshold or -inf)"""
    V1 = zp.size
    comp = ~np.isnan(zp)
    A = comp.copy()
    thr_k = -np.inf
    if top_k not in (0, V1):
        c = np.sort(zp[comp])[::-1]
        if c.size >= top_k:
            thr_k = c[top_k - 1]
            A &= zp >= thr_k
    zmax = zp[comp].max() if comp.any() else -np.inf
    with np.errstate(invalid='ignore'):
        d = np.where(zp == zmax, 0.0, (zp - zmax) / temperature)
    S = A.copy()
    if min_p > 0:
        S &= d >= np.log(min_p)
    ahead = np.zeros(V1)
    F = S.copy()
    if 0 < top_p < 1 and S.any():
        w = np.where(S, np.exp(np.where(S, d, 0.0)), 0.0)
        q = w / w.sum()
        vals, inv = np.unique(zp[S], return_inverse=True)          # ascending distinct z' of the survivors
        mass = np.bincount(inv.reshape(-1), weights=q[S], minlength=vals.size)
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])     # mass of the strictly larger values
        ahead[S] = above[inv.reshape(-1)]
        F &= ahead < top_p
    return dict(A=A, S=S, F=F, d=d, ahead=ahead, thr_k=thr_k, zmax=zmax)


def argmax_comparable(zp):
    comp = ~np.isnan(zp)
    if not comp.any():
        return 0
    return int(np.flatnonzero(zp == zp[comp].max())[0])


def choose(zp, temperature, top_k, top_p, min_p, noise):
    """step 5 on penalised logits -> (token, perturbed scores over the final set (-inf elsewhere), sets or None)"""
    if temperature == 0 or top_k == 1:
        return argmax_comparable(zp), zp.copy(), None
    s = filter_sets(zp, temperature, top_k, top_p, min_p)
    F = s['F']
    score = np.where(F, zp / temperature + noise, -np.inf)
    if not F.any():
        return 0, score, s
    best = score[F].max()
    return int(np.flatnonzero(F & (score == best))[0]), score, s


def generate(params, config, n_seq, num, temperature=1.0, top_k=0, seed=0, primer=None, top_p=0.0, min_p=0.0, theta=1.0, window=0):
    """the free-running fp64 draw with filters: -> tokens int [B, num], log-probs [B, num]"""
    d = O.model_dims(config)
    P = 0 if primer is None else np.asarray(primer).shape[1]
    toks = np.zeros((n_seq, num), np.int64)
    lps = np.zeros((n_seq, num))
    for b in range(n_seq):
        ctx = [] if P == 0 else [int(w) for w in primer[b]]
        lg_all = None
        for t in range(num):
            inputs = [d['start']] + ctx
            lg_all = R.row_logits(params, config, inputs)
            z = lg_all[-1]
            zp = penalise(z, ctx, theta, window)
            w, _, _ = choose(zp, temperature, top_k, top_p, min_p, R.gumbel(seed, t, b, d['V1']))
            toks[b, t] = w
            lps[b, t] = z[w] - R.logsumexp(z)
            ctx.append(w)
    return toks, lps


def check_margins(params, config, toks, lps, temperature, top_k, seed, top_p=0.0, min_p=0.0, theta=1.0, window=0, primer=None,
                  rows=None, tol=1e-4, tie=1e-4):
    """Teacher-forced check of GPU output: feed row b's own token history into the fp64 decoder; at every generated position
    the GPU token lies in the fp64 final set (a column may be in or out only within BOUNDARY of a top-k, min-p or top-p boundary),
    its perturbed score is within tol of the fp64 best over the columns certainly in the set, its log-prob is within tol, and it
    equals the fp64 choice wherever the margin is >= tie and no decision is near a boundary.  -> number of near cases seen."""
    d = O.model_dims(config)
    V1 = d['V1']
    B, num = toks.shape
    P = 0 if primer is None else np.asarray(primer).shape[1]
    near_seen = 0
    for b in (range(B) if rows is None else rows):
        pr = [] if P == 0 else [int(w) for w in primer[b]]
        inputs = [d['start']] + pr + [int(w) for w in toks[b, :-1]]
        lg_all = R.row_logits(params, config, inputs)[P:]
        for t in range(num):
            z, g = lg_all[t], int(toks[b, t])
            assert 0 <= g < V1, (b, t, g)
            zp = penalise(z, pr + [int(w) for w in toks[b, :t]], theta, window)
            noise = R.gumbel(seed, t, b, V1)
            want, score, s = choose(zp, temperature, top_k, top_p, min_p, noise)
            assert abs(float(lps[b, t]) - (z[g] - R.logsumexp(z))) <= tol, ('logprob', b, t, lps[b, t], z[g] - R.logsumexp(z))
            if s is None:
                sg, best, near = zp[g], zp[want], np.zeros(V1, bool)
                certain = None
            else:
                near = np.zeros(V1, bool)
                if np.isfinite(s['thr_k']):
                    near |= np.abs(zp - s['thr_k']) <= BOUNDARY
                if min_p > 0:
                    near |= s['A'] & (np.abs(s['d'] - np.log(min_p)) <= BOUNDARY)
                if 0 < top_p < 1:
                    near |= s['S'] & (np.abs(s['ahead'] - top_p) <= BOUNDARY)
                assert s['F'][g] or near[g], ('outside the final set', b, t, g, zp[g], s['d'][g], s['ahead'][g])
                certain = s['F'] & ~near
                sg = zp[g] / temperature + noise[g]
                best = score[certain].max() if certain.any() else -np.inf
            assert sg >= best - tol, ('margin', b, t, g, want, sg, best)
            fin = score[np.isfinite(score)] if s is not None else score[~np.isnan(score)]
            srt = np.sort(fin)
            margin = srt[-1] - srt[-2] if srt.size > 1 else np.inf
            if margin >= tie and not near.any():
                assert g == want, ('token', b, t, g, want, margin)
            else:
                near_seen += 1
    return near_seen
