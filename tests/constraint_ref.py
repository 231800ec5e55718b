"""numpy restatement of fsmg_generate_constrained (include/fsmg.h "constrained decoding") on top of filter_ref /
gen_ref: the constrained logits z^c, filter_ref.choose on them, the state advance, the primer walk and the dead-end rule; the
free-running decoder in fp64 (or, dtype=np.float32, an fp32 stand-in of the device's arithmetic); and the teacher-forced margin
check the GPU tests use, which extends filter_ref.check_margins and reuses its boundary constant.

`mistake` plants one wrong reading of the contract into the decoder (tests/test_constraints_cpu.py: each must fail the checks)."""
import numpy as np

import filter_ref as F
import gen_ref as R
from oracle import lstm_oracle as O

MISTAKES = ('no_flip_on_close', 'class_of_previous_token', 'bias_after_penalty', 'primer_does_not_advance', 'bit32_in_word0',
            'dead_end_advances', 'omega_after_topk')


def _bias(con):
    return np.zeros(con.n_columns) if con.bias is None else con.bias.astype(np.float64)


def constrained_logits(con, z, state, open_words):
    """-> (z^c, Omega bool [V1], dead): z^c = z + bias over Omega and -inf elsewhere; at a dead end (Omega empty) z itself"""
    ok = con.allowed(state, open_words)
    z = np.asarray(z)
    if not ok.any():
        return z.astype(np.float64), ok, True
    with np.errstate(invalid='ignore'):
        zb = (z.astype(np.float32) + _bias(con).astype(np.float32)).astype(np.float64) if z.dtype == np.float32 else z + _bias(con)
    return np.where(ok, zb, -np.inf), ok, False


def pick(con, z, ctx, state, open_words, temperature, top_k, top_p, min_p, theta, window, noise):
    """one constrained pick -> (token, perturbed scores, filter sets or None, Omega, dead, penalised z^c)"""
    zc, ok, dead = constrained_logits(con, z, state, open_words)
    zp = F.penalise(zc, ctx, theta, window)
    w, score, s = F.choose(zp, temperature, top_k, top_p, min_p, noise)
    if not dead and not (zp[ok] > -np.inf).any():
        w = int(np.flatnonzero(ok)[0])         # no allowed column compares above -inf: the lowest column of Omega
    return w, score, s, ok, dead, zp


def walk_primer(con, primer_row, state, open_words):
    """the state after the primer tokens, in order; -> (state, open, index of the first token that is not allowed, or None)"""
    s, o = int(state), np.array(open_words, np.uint32)
    for i, w in enumerate(primer_row):
        if not con.token_allowed(s, o, w):
            return s, o, i
        s, o = con.advance(s, o, w)
    return s, o, None


def _fp(dtype, x):
    return np.asarray(x, dtype)


def _row_logits(params, config, inputs, dtype):
    if dtype == np.float64:
        return R.row_logits(params, config, inputs)
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    p = {k: _fp(dtype, v) for k, v in params.items()}
    hs = [np.zeros(H, dtype) for _ in range(L)]
    cs = [np.zeros(H, dtype) for _ in range(L)]
    fb, one = dtype(O.FORGET_BIAS), dtype(1)
    sig = lambda x: one / (one + np.exp(-x))
    out = []
    for w in inputs:
        x = p['embedding'][w]
        for l in range(L):
            z = np.concatenate([x, hs[l]]).dot(p['kernel_%d' % l]) + p['bias_%d' % l]
            i, j, f, o = z[:H], z[H:2 * H], z[2 * H:3 * H], z[3 * H:]
            cs[l] = cs[l] * sig(f + fb) + sig(i) * np.tanh(j)
            hs[l] = np.tanh(cs[l]) * sig(o)
            x = hs[l]
        out.append(x.dot(p['softmax_w']) + p['softmax_b'])
    return np.stack(out)


def initial_cstate(con, n_seq, cstate=None):
    cs = cstate or {}
    state = np.full(n_seq, con.start_state, np.int32) if cs.get('state') is None else np.array(cs['state'], np.int32)
    opn = (np.zeros((n_seq, con.n_words), np.uint32) if cs.get('open') is None
           else np.array(cs['open'], np.uint32).reshape(n_seq, con.n_words))
    dead = np.zeros(n_seq, np.int32) if cs.get('dead_ends') is None else np.array(cs['dead_ends'], np.int32)
    return state, opn, dead


def generate(params, config, con, n_seq, num, temperature=1.0, top_k=0, seed=0, primer=None, top_p=0.0, min_p=0.0, theta=1.0, window=0,
             cstate=None, dtype=np.float64, mistake=None, t0=0, context=None):
    """the free-running constrained draw -> tokens int [B, num], log-probs [B, num], cstate dict.  t0: the Philox position of the
    first token (a continued call); context: per row, the tokens read before this call (a continued call's history, behind the
    primer).  dtype=np.float32: the model and the constrained logits in fp32."""
    assert mistake is None or mistake in MISTAKES, mistake
    d = O.model_dims(config)
    V1 = d['V1']
    P = 0 if primer is None else np.asarray(primer).shape[1]
    toks = np.zeros((n_seq, num), np.int64)
    lps = np.zeros((n_seq, num))
    state, opn, deads = initial_cstate(con, n_seq, cstate)
    for b in range(n_seq):
        ctx = ([] if context is None else [int(w) for w in context[b]]) + ([] if P == 0 else [int(w) for w in primer[b]])
        s, o = int(state[b]), opn[b].copy()
        if P and mistake != 'primer_does_not_advance':
            s, o, bad = walk_primer(con, primer[b], s, o)
            assert bad is None, ('primer token not allowed', b, bad)
        prev = None
        for t in range(num):
            z = _row_logits(params, config, [d['start']] + ctx, dtype)[-1]
            noise = R.gumbel(seed, t0 + t, b, V1)
            if dtype != np.float64:
                noise = noise.astype(dtype).astype(np.float64)
            if mistake == 'bias_after_penalty' and con.bias is not None:
                ok = con.allowed(s, o)
                dead = not ok.any()
                zp = F.penalise(z, ctx, theta, window)
                zp = zp if dead else np.where(ok, zp + _bias(con), -np.inf)
                w, _, _ = F.choose(zp, temperature, top_k, top_p, min_p, noise)
            elif mistake == 'omega_after_topk':
                ok = con.allowed(s, o)
                dead = not ok.any()
                zp = F.penalise(np.asarray(z, np.float64) + (0 if dead else np.where(np.isfinite(_bias(con)), _bias(con), 0.0)), ctx, theta,
                                window)
                if temperature == 0 or top_k == 1 or dead:
                    w = F.argmax_comparable(zp if dead else np.where(ok, zp, -np.inf))
                else:
                    fs = F.filter_sets(zp, temperature, top_k, top_p, min_p)
                    keep = fs['F'] & ok
                    score = np.where(keep, zp / temperature + noise, -np.inf)
                    w = int(np.argmax(score)) if keep.any() else int(np.flatnonzero(ok)[0])
            else:
                w, _, _, ok, dead, _ = pick(con, z, ctx, s, o, temperature, top_k, top_p, min_p, theta, window, noise)
            toks[b, t] = w
            z64 = np.asarray(z, np.float64)
            lps[b, t] = z64[w] - R.logsumexp(z64)
            if dead and mistake != 'dead_end_advances':
                deads[b] += 1
            else:
                if dead:
                    deads[b] += 1
                cls_tok = prev if (mistake == 'class_of_previous_token' and prev is not None) else w
                s2, o2 = con.advance(s, o, w)
                if con.token_class is not None:
                    s2 = int(con.next_state[s, con.token_class[cls_tok]])
                    s2 = s if s2 < 0 else s2
                if mistake == 'no_flip_on_close' and con.slot_close is not None and con.slot_close[w] >= 0:
                    o2 = o.copy()
                if mistake == 'bit32_in_word0':
                    for a in (con.slot_open, con.slot_close):
                        if a is not None and a[w] == 32:
                            o2 = o.copy()
                            o2[0] ^= np.uint32(1)
                s, o = s2, o2
            prev = w
            ctx.append(w)
        state[b], opn[b] = s, o
    return toks, lps, dict(state=state, open=opn, dead_ends=deads)


def check_margins(params, config, con, toks, lps, temperature, top_k, seed, top_p=0.0, min_p=0.0, theta=1.0, window=0, primer=None,
                  rows=None, cstate_in=None, cstate_out=None, tol=1e-4, tie=1e-4, t0=0, context=None):
    """filter_ref.check_margins under a constraint: row b's own tokens are fed into the fp64 decoder and its constraint state is
    walked along.  At every generated position: exactly, the token lies in Omega (any column at a dead end); within tolerance, it
    lies in the fp64 final set of z^c (in or out only within filter_ref.BOUNDARY of a top-k, min-p or top-p boundary), its
    perturbed score is within tol of the fp64 best, its log-prob (from the raw z) is within tol, and it equals the fp64 choice
    wherever the margin is >= tie and no decision is near a boundary.  cstate_out: the returned states, compared exactly with the
    walked ones (state, open bits, dead ends).  -> number of near cases seen."""
    d = O.model_dims(config)
    V1 = d['V1']
    B, num = toks.shape
    P = 0 if primer is None else np.asarray(primer).shape[1]
    state, opn, deads = initial_cstate(con, B, cstate_in)
    near_seen = 0
    for b in (range(B) if rows is None else rows):
        hist = [] if context is None else [int(w) for w in context[b]]
        pr = [] if P == 0 else [int(w) for w in primer[b]]
        s, o, bad = walk_primer(con, pr, state[b], opn[b])
        assert bad is None, ('primer token not allowed', b, bad)
        inputs = [d['start']] + hist + pr + [int(w) for w in toks[b, :-1]]
        lg_all = R.row_logits(params, config, inputs)[len(hist) + P:]
        n_dead = int(deads[b])
        for t in range(num):
            z, g = lg_all[t], int(toks[b, t])
            assert 0 <= g < V1, (b, t, g)
            noise = R.gumbel(seed, t0 + t, b, V1)
            want, score, fs, ok, dead, zp = pick(con, z, hist + pr + [int(w) for w in toks[b, :t]], s, o, temperature, top_k, top_p, min_p,
                                                 theta, window, noise)
            assert dead or ok[g], ('outside Omega', b, t, g, s)
            assert abs(float(lps[b, t]) - (z[g] - R.logsumexp(z))) <= tol, ('logprob', b, t, lps[b, t], z[g] - R.logsumexp(z))
            flat = not dead and not (zp[ok] > -np.inf).any()
            if flat:
                assert g == want, ('lowest column of Omega', b, t, g, want)
            elif fs is None:
                sg, best, near = zp[g], zp[want], np.zeros(V1, bool)
                assert sg >= best - tol, ('margin', b, t, g, want, sg, best)
            else:
                near = np.zeros(V1, bool)
                if np.isfinite(fs['thr_k']):
                    near |= np.abs(zp - fs['thr_k']) <= F.BOUNDARY
                if min_p > 0:
                    near |= fs['A'] & (np.abs(fs['d'] - np.log(min_p)) <= F.BOUNDARY)
                if 0 < top_p < 1:
                    near |= fs['S'] & (np.abs(fs['ahead'] - top_p) <= F.BOUNDARY)
                assert fs['F'][g] or near[g], ('outside the final set', b, t, g, zp[g], fs['d'][g], fs['ahead'][g])
                certain = fs['F'] & ~near
                sg = zp[g] / temperature + noise[g]
                best = score[certain].max() if certain.any() else -np.inf
                assert sg >= best - tol, ('margin', b, t, g, want, sg, best)
            if not flat:
                fin = score[np.isfinite(score)] if fs is not None else score[~np.isnan(score) & (score > -np.inf)]
                srt = np.sort(fin)
                margin = srt[-1] - srt[-2] if srt.size > 1 else np.inf
                if margin >= tie and not near.any():
                    assert g == want, ('token', b, t, g, want, margin)
                else:
                    near_seen += 1
            if dead:
                n_dead += 1
            else:
                s, o = con.advance(s, o, g)
        if cstate_out is not None:
            assert int(cstate_out['state'][b]) == s, ('state', b, int(cstate_out['state'][b]), s)
            assert np.array_equal(np.asarray(cstate_out['open'], np.uint32).reshape(B, -1)[b], o), ('open', b)
            assert int(cstate_out['dead_ends'][b]) == n_dead, ('dead_ends', b, int(cstate_out['dead_ends'][b]), n_dead)
    return near_seen


def mixed_constraint(V1, K=33, seed=0, S=3, C=4, ban=0.1):
    """bias, automaton and slots together over V1 columns (the tests' general case): a finite random bias with a fraction `ban` of
    the columns (the start word among them) banned; an S-state automaton over C classes that forbids one class per state (never
    class 0, so no state is a dead end by itself); the first K even columns open slots 0 .. K - 1 and the following odd ones
    close them"""
    from data.constraints import Constraints
    rs = np.random.RandomState(seed)
    bias = rs.randn(V1).astype(np.float32)
    bias[rs.rand(V1) < ban] = -np.inf
    bias[V1 - 1] = -np.inf
    token_class = rs.randint(0, C, size=V1).astype(np.int32)
    next_state = rs.randint(0, S, size=(S, C)).astype(np.int32)
    for s in range(S):
        if C > 1:
            next_state[s, 1 + (s % (C - 1))] = -1
    K = min(K, (V1 - 1) // 2)
    slot_open = np.full(V1, -1, np.int32)
    slot_close = np.full(V1, -1, np.int32)
    slot_open[0:2 * K:2] = np.arange(K)
    slot_close[1:2 * K:2] = np.arange(K)
    return Constraints(V1, bias=bias, token_class=token_class, next_state=next_state, start_state=S - 1, slot_open=slot_open,
                       slot_close=slot_close, n_slots=K)


def allowed_primer(con, n_rows, P, seed=0):
    """n_rows random primers of P tokens, each token allowed where it stands (never the start word: the last column)"""
    rs = np.random.RandomState(seed)
    out = np.zeros((n_rows, P), np.int32)
    for b in range(n_rows):
        s, o = con.initial()
        for p in range(P):
            ok = con.allowed(s, o)
            ok[-1] = False
            w = int(rs.choice(np.flatnonzero(ok)))
            out[b, p] = w
            s, o = con.advance(s, o, w)
    return out
