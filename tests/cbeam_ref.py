"""numpy restatement of fsmg_beam_search_constrained (include/fsmg.h "constrained beam search") on top of beam_ref and
constraint_ref, and the checks the GPU tests use.

Every slot carries (h, c, state, open, dead).  A slot whose allowed set Omega is not empty offers the columns of Omega only, with
z^c = z + bias, lp = z^c - lse and s = cum + lp; a slot at a dead end offers all V1 columns with z^c = z, in a lower tier.  A group's
candidates rank by tier (live slots first), then s descending, j ascending, z^c descending, v ascending, NaN below -inf.  A winner
from a live slot takes its parent's state advanced by its token; one from a dead-end slot its parent's state unchanged and one more
dead end.

dtype=np.float32 is a stand-in of the device's arithmetic (the model, z^c, lp and s in fp32).  `mistake` plants one wrong reading
of the contract (tests/test_cbeam_cpu.py: each must fail a check)."""
import numpy as np

import beam_ref as BR
import constraint_ref as CR
from oracle import lstm_oracle as O

MISTAKES = ('slot_keeps_own_state', 'open_not_reordered', 'no_tier', 'excluded_as_minus_inf', 'bias_not_in_score',
            'dead_end_advances', 'advance_by_parent_token')


def _cell_step(p, H, L, x, hs, cs, dtype):
    fb, one = dtype(O.FORGET_BIAS), dtype(1)
    sig = lambda a: one / (one + np.exp(-a))
    for l in range(L):
        z = np.concatenate([x, hs[l]]).dot(p['kernel_%d' % l]) + p['bias_%d' % l]
        i, j, f, o = z[:H], z[H:2 * H], z[2 * H:3 * H], z[3 * H:]
        cs[l] = cs[l] * sig(f + fb) + sig(i) * np.tanh(j)
        hs[l] = np.tanh(cs[l]) * sig(o)
        x = hs[l]
    return x.dot(p['softmax_w']) + p['softmax_b']


def _advance(con, s, o, v):
    """con.advance, except that a forbidden class leaves the state where it is (only a planted mistake gets there)"""
    s2, o2 = con.advance(s, o, v)
    return (s if s2 < 0 else s2), o2


def row_candidates(con, z, lse, cum, s, o, W, dtype=np.float64, mistake=None):
    """one slot's W + 1 best candidates in the row's own order (z^c descending, NaN lowest, v ascending: lp and s are
    nondecreasing in z^c, so no other candidate of the row can be among the group's first W + 1)
    -> (dead, columns, z^c, lp, s)"""
    V1 = con.n_columns
    z = np.asarray(z, dtype)
    ok = con.allowed(s, o)
    dead = not ok.any()
    bias = CR._bias(con).astype(dtype)
    with np.errstate(invalid='ignore'):
        if dead:
            cols, zc = np.arange(V1), z
        elif mistake == 'excluded_as_minus_inf':
            cols, zc = np.arange(V1), np.where(ok, z + bias, dtype(-np.inf)).astype(dtype)
        elif mistake == 'bias_not_in_score':
            cols = np.flatnonzero(ok)
            zc = z[cols]
        else:
            cols = np.flatnonzero(ok)
            zc = (z + bias).astype(dtype)[cols]
        lp = (zc - dtype(lse)).astype(dtype)
        sc = (dtype(cum) + lp).astype(dtype)
    nan = np.isnan(zc)
    key = np.where(nan, 0.0, -zc.astype(np.float64))
    idx = np.lexsort((cols, key, nan))[:W + 1]
    return dead, cols[idx], zc[idx], lp[idx], sc[idx]


def _key(tier, j, v, zc, s):
    s, zc = float(s), float(zc)
    return (tier, s != s, 0.0 if s != s else -s, j, zc != zc, 0.0 if zc != zc else -zc, int(v))


def rank_group(rows, W, mistake=None):
    """rows: row_candidates' result per slot -> (the group's first W + 1 candidates as (tier, j, v, lp, s), best first; the
    smallest score gap between adjacent candidates of the same tier among them)"""
    cands = []
    for j, (dead, cols, zc, lp, sc) in enumerate(rows):
        tier = 1 if dead and mistake != 'no_tier' else 0
        for v, a, b, c in zip(cols, zc, lp, sc):
            cands.append((_key(tier, j, v, a, c), (tier, j, int(v), b, c)))
    cands.sort(key=lambda x: x[0])
    first = [c for _, c in cands[:W + 1]]
    gap = np.inf
    for a, b in zip(first[:-1], first[1:]):
        if a[0] == b[0] and np.isfinite(a[4]) and np.isfinite(b[4]):
            gap = min(gap, abs(float(a[4]) - float(b[4])))
    return first, gap


def beam_search(params, config, con, n_groups, W, num, primer=None, cstate=None, dtype=np.float64, mistake=None):
    """-> tokens int [G, W, num], scores [G, W], lps [G, W, num], gaps [G, num], cstate dict of 'state' [G, W], 'open' [G, W, words],
    'dead_ends' [G, W] (the hypotheses' final constraint states).  cstate: the groups' states to start from ([G] each)."""
    assert mistake is None or mistake in MISTAKES, mistake
    d = O.model_dims(config)
    H, L = d['H'], d['L']
    p = {k: np.asarray(v, dtype) for k, v in params.items()}
    P = 0 if primer is None else np.asarray(primer).shape[1]
    toks = np.zeros((n_groups, W, num), np.int64)
    lps = np.zeros((n_groups, W, num), dtype)
    scores = np.zeros((n_groups, W), dtype)
    gaps = np.zeros((n_groups, num))
    st0, op0, de0 = CR.initial_cstate(con, n_groups, cstate)
    out = dict(state=np.zeros((n_groups, W), np.int32), open=np.zeros((n_groups, W, con.n_words), np.uint32),
               dead_ends=np.zeros((n_groups, W), np.int32))
    for g in range(n_groups):
        hs = [np.zeros(H, dtype) for _ in range(L)]
        cs = [np.zeros(H, dtype) for _ in range(L)]
        pr = [] if P == 0 else [int(w) for w in primer[g]]
        inputs = [d['start']] + pr
        for w in inputs[:-1]:
            _cell_step(p, H, L, p['embedding'][w], hs, cs, dtype)
        s, o, bad = CR.walk_primer(con, pr, st0[g], op0[g])
        assert bad is None, ('primer token not allowed', g, bad)
        # a slot: h, c, the token it reads next, constraint state, open bits, dead ends, tokens, lps
        slots = [dict(h=[x.copy() for x in hs], c=[x.copy() for x in cs], w=inputs[-1], s=int(s), o=o.copy(), dead=int(de0[g]), tk=[], lk=[])
                 for _ in range(W)]
        cum = np.array([0.0] + [-np.inf] * (W - 1), dtype)
        for t in range(num):
            rows = []
            for j, sl in enumerate(slots):
                z = _cell_step(p, H, L, p['embedding'][sl['w']], sl['h'], sl['c'], dtype)
                rows.append(row_candidates(con, z, BR.lse_of(z, dtype), cum[j], sl['s'], sl['o'], W, dtype, mistake))
            first, gaps[g, t] = rank_group(rows, W, mistake)
            new = []
            for n, (_, j, v, lp, sc) in enumerate(first[:W]):
                par, own = slots[j], slots[n]
                src = own if mistake == 'slot_keeps_own_state' else par
                s_in, o_in, dead_in = src['s'], (own['o'] if mistake == 'open_not_reordered' else src['o']), src['dead']
                by = par['w'] if mistake == 'advance_by_parent_token' else v
                if rows[j][0]:          # the parent stands at a dead end
                    s2, o2 = _advance(con, s_in, o_in, by) if mistake == 'dead_end_advances' else (s_in, o_in.copy())
                    dead2 = dead_in + 1
                else:
                    s2, o2 = _advance(con, s_in, o_in, by)
                    dead2 = dead_in
                new.append(dict(h=[x.copy() for x in par['h']], c=[x.copy() for x in par['c']], w=v, s=int(s2), o=o2, dead=dead2,
                                tk=par['tk'] + [v], lk=par['lk'] + [lp]))
            cum = np.array([c[4] for c in first[:W]], dtype)
            slots = new
        for n, sl in enumerate(slots):
            toks[g, n], lps[g, n] = sl['tk'], sl['lk']
            out['state'][g, n], out['open'][g, n], out['dead_ends'][g, n] = sl['s'], sl['o'], sl['dead']
        scores[g] = cum
    return toks, scores, lps, gaps, out


# ---------------------------------------------------------------------------------------------- the checks the GPU tests use
def check_walk(con, toks, scores, lps, cs_out, primer=None, cs_in=None):
    """exactly: every hypothesis, walked with Constraints from its group's start state over primer and tokens, draws from its Omega
    (any column at a dead end) and ends in the returned state, open bits and dead ends; its score is the fp32 left-to-right sum of
    its log-probs, bitwise; finite-scored hypotheses of a group are distinct; scores do not increase among the hypotheses that met
    no dead end, and those come first"""
    G, W, num = toks.shape
    state, opn, dead = CR.initial_cstate(con, G, cs_in)
    for g in range(G):
        s0, o0, bad = CR.walk_primer(con, [] if primer is None else primer[g], state[g], opn[g])
        assert bad is None, ('primer', g, bad)
        met = []
        for n in range(W):
            s, o, n_dead = s0, o0.copy(), int(dead[g])
            for t, v in enumerate(toks[g, n].tolist()):
                assert 0 <= v < con.n_columns, (g, n, t, v)
                if con.allowed(s, o).any():
                    assert n_dead == int(dead[g]), ('a dead end was left', g, n, t)
                    assert con.token_allowed(s, o, v), ('outside Omega', g, n, t, v, s)
                    s, o = con.advance(s, o, v)
                else:
                    n_dead += 1
            assert int(cs_out['state'][g, n]) == s, ('state', g, n, int(cs_out['state'][g, n]), s)
            assert int(cs_out['dead_ends'][g, n]) == n_dead, ('dead_ends', g, n, int(cs_out['dead_ends'][g, n]), n_dead)
            assert np.array_equal(np.asarray(cs_out['open'], np.uint32).reshape(G, W, -1)[g, n], o), ('open', g, n)
            assert BR.fp32_sum(lps[g, n]).view(np.uint32) == np.float32(scores[g, n]).view(np.uint32), ('score', g, n)
            met.append(n_dead - int(dead[g]))
        finite = [tuple(toks[g, n]) for n in range(W) if np.isfinite(scores[g, n])]
        assert len(set(finite)) == len(finite), ('not distinct', g)
        live = [n for n in range(W) if met[n] == 0]
        assert live == list(range(len(live))), ('dead-end hypotheses first', g, met)
        sc = np.asarray(scores[g], np.float64)[live]
        assert not np.any(np.diff(sc[~np.isnan(sc)]) > 0), ('not sorted', g, scores[g])


def check_against(ref, toks, scores, cs_out, tol, num):
    """ref = beam_search(...) in fp64: every group whose fp64 gaps all exceed tol must equal the reference's hypotheses, order and
    dead ends, its scores within tol * num -> (clear groups, groups)"""
    rt, rs, _, gaps, rc = ref
    clear = 0
    for g in range(rt.shape[0]):
        if not np.all(gaps[g] > tol):
            continue
        clear += 1
        assert np.array_equal(toks[g], rt[g]), (g, toks[g], rt[g])
        assert np.array_equal(cs_out['dead_ends'][g], rc['dead_ends'][g]), (g, cs_out['dead_ends'][g], rc['dead_ends'][g])
        both = np.isfinite(rs[g])
        assert np.array_equal(np.isfinite(np.asarray(scores[g], np.float64)), both), (g, scores[g], rs[g])
        assert np.max(np.abs(np.asarray(scores[g], np.float64)[both] - rs[g][both]), initial=0.0) <= tol * num, (g, scores[g], rs[g])
    return clear, rt.shape[0]


# ---------------------------------------------------------------------------------------------- the tests' shared inputs
REF_CASES = ((3, 4, 0), (2, 16, 4), (2, 64, 0), (3, 4, 6), (2, 16, 0), (2, 64, 3))       # (G, W, P), tests/test_beam.py's
REF_SHAPES = ((24, 1), (200, 2), (512, 1), (1024, 2))                                     # H x L


def ref_config(H, L, input_size=300):
    return dict(input_size=input_size, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)


def ref_params(cfg, seed):
    """fp32-representable parameters from numpy alone: Glorot, softmax_w * 40, softmax_b = N(0, 2) -- a wide spread of
    state-dependent logits, so that most gaps between adjacent ranks are clear"""
    p = {k: np.asarray(v, np.float32) for k, v in O.glorot_init(cfg, seed=seed).items()}
    p['softmax_w'] = (p['softmax_w'] * np.float32(40)).astype(np.float32)
    p['softmax_b'] = (np.random.RandomState(seed).randn(cfg['input_size'] + 1) * 2).astype(np.float32)
    return p


def f64(params):
    return {k: np.asarray(v, np.float64) for k, v in params.items()}


def dead_end_constraint(all_dead=False, V1=98):
    """bias -inf everywhere except bias[10] = -5, bias[20] = bias[30] = 0; columns 20 and 30 have class 1; state 0 goes to state 1
    on class 1 and stays on class 0, state 1 allows nothing.  all_dead: state 0 forbids class 0 too, so only 20 and 30 are allowed
    at the first position and every hypothesis stands at a dead end from the second on"""
    from data.constraints import Constraints
    bias = np.full(V1, -np.inf, np.float32)
    bias[10], bias[20], bias[30] = -5.0, 0.0, 0.0
    cls = np.zeros(V1, np.int32)
    cls[20] = cls[30] = 1
    nxt = np.array([[-1, 1], [-1, -1]] if all_dead else [[0, 1], [-1, -1]], np.int32)
    return Constraints(V1, bias=bias, token_class=cls, next_state=nxt)


def slot_dead_end_constraint(V1=98):
    """a dead end through the slots: column v opens slot v % 2 and nothing closes one; only columns 0 and 1 pass the bias.  After
    both are drawn nothing is allowed, and a token drawn at the dead end must leave the open bits alone"""
    from data.constraints import Constraints
    bias = np.full(V1, -np.inf, np.float32)
    bias[0] = bias[1] = 0.0
    return Constraints(V1, bias=bias, slot_open=np.arange(V1, dtype=np.int32) % 2, n_slots=2)
