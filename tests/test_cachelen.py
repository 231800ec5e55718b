"""Per-song lengths in scoring and in the support-set cache (fsmg_*_masked, ragged cache groups) on the MI355X.

The tests rest on bitwise laws whose reference is the existing, already verified unmasked path, so they need no tolerance:
  1. full lengths     every output of every _masked call is the unmasked call's bits; a masked-built cache has counts all Mg
  2. padding          replacing the tokens at t >= len by other in-range ids changes no output bit, cache contents included
  3. entries          group g of a masked-built cache holds, in order, exactly the entries (row, t < len) of the unmasked build
  4. trim             every consumer gives for group g of a ragged cache the bits it gives on a uniform one-group cache made of
                      g's first n_g entries
  5. prefix           scored positions equal the unmasked call, unscored ones are exactly 0, row_nll is recomputable
Against fp64 (tests/cachelen_ref.py) the bounds are test_cache's own: max(8 * e32, 1e-6) for the attention, 1e-4 on the model's
log-prob and 1e-4 + theta * 2e-5 * l1 on the mixture."""
import ctypes as C
import functools

import numpy as np
import pytest

import cache_ref as R
import cachelen_ref as CL
import masked_ref as MR
from conftest import small_config
from gpu_utils import new_model
from gpu_utils import f64_params
from oracle import lstm_oracle as O
from test_cache import SHAPES, N_TOKENS, _attend_model, _check_attend, _episode_rows, _rel_err, _same, _thetas_for

pytestmark = pytest.mark.gpu

CAP = 80                                    # the capacity of the kernel-level caches
COUNT_PAIRS = ((1, 80), (15, 65), (16, 64), (17, 63))      # the 16-key tile and the four-wave round of 64, two groups per call


def _ragged_arrays(rng, H, counts, cap=CAP, negative=False):
    """host arrays of a ragged cache: real entries in front, and behind each count LARGE POSITIVE keys with out-of-range values --
    a dead slot that was read, or scored, would show"""
    G = len(counts)
    keys = rng.normal(size=(G, cap, H)) / np.sqrt(H)
    keys = (-np.abs(keys) if negative else keys).astype(np.float32)
    vals = rng.randint(0, N_TOKENS, size=(G, cap)).astype(np.int32)
    for g, n in enumerate(counts):
        keys[g, n:] = 50.0 + np.abs(keys[g, n:])
        vals[g, n:] = 999
    return keys, vals


def _trimmed(m, keys, vals, counts):
    """one uniform one-group cache per group, out of its first n_g entries"""
    return [m.cache_from(keys[g:g + 1, :n], vals[g:g + 1, :n]) for g, n in enumerate(counts)]


def _close(caches):
    for c in caches:
        c.close()


# ------------------------------------------------------------------------------------------------ attend
@pytest.mark.parametrize('H', [24, 200, 512])
def test_attend_walks_the_count_not_the_capacity(H):
    m = _attend_model(H)
    for counts in COUNT_PAIRS:
        rng = np.random.RandomState(100 * counts[0] + H)
        keys, vals = _ragged_arrays(rng, H, counts)
        ragged = m.cache_from(keys, vals, counts=counts)
        assert np.array_equal(ragged.counts(), counts) and ragged.info()['entries'] == CAP
        k, v = ragged.get()
        for g, n in enumerate(counts):
            assert _same(k[g, :n], keys[g, :n]) and np.array_equal(v[g, :n], vals[g, :n])
            assert not k[g, n:].any() and not v[g, n:].any()                # what lies behind the count reads back as zeros
        trimmed = _trimmed(m, keys, vals, counts)
        for n in (1, 17, 33):
            q = rng.normal(size=(n, H)).astype(np.float32) * 3
            group = (np.arange(n) % 2).astype(np.int32) if n > 1 else np.array([1 if counts[0] == 1 else 0], np.int32)
            y = np.array([vals[g, rng.randint(0, counts[g])] for g in group], np.int32)
            if n > 1:
                y[1] = N_TOKENS                                             # a target no entry holds
            thetas = _thetas_for(keys[:1, :counts[0]], q)
            got = m.cache_attend(ragged, q, y, thetas, group=group)
            assert _same(got, m.cache_attend(ragged, q, y, thetas, group=group))
            for g in range(2):
                sel = np.flatnonzero(group == g)
                if sel.size:
                    assert _same(got[:, sel], m.cache_attend(trimmed[g], q[sel], y[sel], thetas)), (counts, n, g)
                    _check_attend('H %d counts %r n %d g %d' % (H, counts, n, g), got[:, sel], keys[g:g + 1, :counts[g]],
                                  vals[g:g + 1, :counts[g]], q[sel], y[sel], None, thetas)
            assert np.all(got[:, y == N_TOKENS] == 0.0)
        # the self-cache over the union: the support walk by the count, the own-tile round robin continuing from it
        vec = rng.normal(size=(4, 9, H)).astype(np.float32)
        val = rng.randint(0, N_TOKENS, size=(4, 9)).astype(np.int32)
        grp = np.array([0, 1, 1, 0], np.int32)
        both = m.cache_self_attend(vec, val, [0.0, 1.0], 5, cache=ragged, group=grp)
        for g in range(2):
            sel = np.flatnonzero(grp == g)
            assert _same(both[:, sel], m.cache_self_attend(vec[sel], val[sel], [0.0, 1.0], 5, cache=trimmed[g])), (counts, g)
        _close(trimmed + [ragged])


@pytest.mark.parametrize('H', [24, 200, 512])
def test_dead_slots_never_score(H):
    """keys = -|.| against queries = +|.| with theta d <= -5 (test_attend_all_scores_negative_masks_the_tail's inputs): a dead slot
    scored as the zero key it holds on the device would take nearly all the mass"""
    m = _attend_model(H)
    for counts in COUNT_PAIRS:
        rng = np.random.RandomState(counts[0] + 7 * H)
        keys, vals = _ragged_arrays(rng, H, counts, negative=True)
        q = np.abs(rng.normal(size=(17, H))).astype(np.float32)
        group = (np.arange(17) % 2).astype(np.int32)
        y = np.array([vals[g, rng.randint(0, counts[g])] for g in group], np.int32)      # every target has a hit
        d = max(float(q.astype(np.float64).dot(keys[g, :n].astype(np.float64).T).max()) for g, n in enumerate(counts))
        assert d < 0
        theta = float(np.float32(5.001 / -d))
        ragged = m.cache_from(keys, vals, counts=counts)
        trimmed = _trimmed(m, keys, vals, counts)
        got = m.cache_attend(ragged, q, y, [theta, 2 * theta], group=group)
        assert np.all(got > 0)
        for g in range(2):
            sel = np.flatnonzero(group == g)
            assert _same(got[:, sel], m.cache_attend(trimmed[g], q[sel], y[sel], [theta, 2 * theta])), (counts, g)
            _check_attend('negative H %d counts %r g %d' % (H, counts, g), got[:, sel], keys[g:g + 1, :counts[g]],
                          vals[g:g + 1, :counts[g]], q[sel], y[sel], None, [theta, 2 * theta])
            if counts[g] == 1:
                assert np.all(got[:, sel] == 1.0)
        _close(trimmed + [ragged])


# ------------------------------------------------------------------------------------------------ distribution / mix
def test_distribution_and_mix_over_the_count():
    H, cap, counts = 24, 64, (1, 16, 17, 33, 48)
    m = _attend_model(H)
    V1 = 21
    rng = np.random.RandomState(9)
    keys, vals = _ragged_arrays(rng, H, counts, cap=cap)
    vals[4, :40] = 3                                # more than CACHE_MIX_SHORT = 32 of one value within the count: a long segment
    for g, n in enumerate(counts):
        vals[g, n:] = 3                             # ... and the same value behind every count, under a huge key
    assert (vals[4, :48] == 3).sum() > 32
    ragged = m.cache_from(keys, vals, counts=counts)
    trimmed = _trimmed(m, keys, vals, counts)
    n = 10
    q = rng.normal(size=(n, H)).astype(np.float32) * 3
    z = rng.normal(size=(n, V1)).astype(np.float32)
    group = (np.arange(n) % 5).astype(np.int32)
    theta, lam = 1.5, 0.25
    got = m.cache_distribution(ragged, q, z, theta, lam, group=group)
    sk = rng.normal(size=(n, 6, H)).astype(np.float32)
    sv = rng.randint(0, N_TOKENS, size=(n, 6)).astype(np.int32)
    sl = rng.randint(0, 7, size=n).astype(np.int32)
    both = m.cache_self_distribution(q, z, sk, sv, sl, theta, lam, 4, cache=ragged, group=group)
    for g in range(5):
        sel = np.flatnonzero(group == g)
        want = m.cache_distribution(trimmed[g], q[sel], z[sel], theta, lam)
        want2 = m.cache_self_distribution(q[sel], z[sel], sk[sel], sv[sel], sl[sel], theta, lam, 4, cache=trimmed[g])
        for key in ('cache_prob', 'logprob', 'lse'):
            assert _same(got[key][sel], want[key]), (g, key)
            assert _same(both[key][sel], want2[key]), (g, key)
        # p_cache against fp64 on the trimmed entries, and its rows sum to 1: both within the fp32 restatement's own error
        cols = np.arange(V1)
        for i in sel:
            args = (keys[g, :counts[g]], vals[g, :counts[g]], np.repeat(q[i:i + 1], V1, axis=0), cols, [theta])
            p64, p32 = R.attend(*args)[0], R.attend(*args, dtype=np.float32)[0]
            e32 = _rel_err(p32, p64)
            assert _rel_err(got['cache_prob'][i], p64) <= max(8 * e32, 1e-6), (g, i)
            s32 = abs(float(p32.astype(np.float64).sum()) - 1.0)
            assert abs(float(got['cache_prob'][i].astype(np.float64).sum()) - 1.0) <= max(8 * s32, 8 * e32, 1e-6), (g, i)
    _close(trimmed + [ragged])


# ------------------------------------------------------------------------------------------------ build / score / self-score / eval
SUPPORT_LENS = {'15+17': (5, 5, 5, 6, 6, 5), '16+30': (1, 10, 5, 10, 10, 10)}
QUERY_LEN = np.array([10, 1, 5, 9, 2], np.int32)
THETAS, LAMBDAS = [0.0, 2.0, 9.0], [0.0, 0.25, 1.0]
ALL = dict(logprob=True, cache_prob=True, lstm_logprob=True, row_nll=True)


@functools.lru_cache(maxsize=None)
def _shape(name):
    """test_cache._shape at max_len 10 -- the shape's sizes, the ORACLE's parameters (its initialiser and three of its train
    steps), one model per shape for every test of this file -> (cfg, model, the uploaded parameters in fp64)"""
    cfg = small_config(**dict(SHAPES[name], max_len=10))
    params = O.glorot_init(cfg, cfg['seed'])
    opt = O.new_opt_state(params)
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=7):
        O.train_step(params, opt, sup, qry, cfg)
    m = new_model(cfg, params=params)
    return cfg, m, f64_params(m)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    cfg, _, params = _shape(name)
    support, query, _ = _episode_rows(cfg)
    return CL.oracle_pass(params, support, query, cfg)


def _prefix(tag, masked, plain, keep, lens, nll_first=0, nll_count=0):
    """law 5 for one cache_score-shaped dict"""
    for key in ('logprob', 'cache_prob', 'lstm_logprob'):
        assert _same(masked[key][..., keep], plain[key][..., keep]), (tag, key)
        dead = masked[key][..., ~keep]
        assert not dead.any() and not np.signbit(dead).any(), (tag, key)
    assert _same(masked['row_nll'], CL.row_nll(masked['logprob'], lens, nll_first, nll_count)), tag


@pytest.mark.parametrize('lens', list(SUPPORT_LENS))
@pytest.mark.parametrize('name', ['H24', 'H200x2', 'H512'])
def test_build_score_self_score_and_eval_with_lengths(name, lens):
    cfg, m, _ = _shape(name)
    support, query, group = _episode_rows(cfg)
    T, H, V = cfg['max_len'], cfg['hidden_size'], cfg['input_size']
    assert T == 10
    sl = np.array(SUPPORT_LENS[lens], np.int32)
    ql = QUERY_LEN
    counts = [int(sl[:3].sum()), int(sl[3:].sum())]
    assert counts == [int(x) for x in lens.split('+')]
    keep = CL.scored(ql, T)
    full6, full5 = np.full(6, T, np.int32), np.full(5, T, np.int32)

    # ---- law 1: full lengths are the unmasked calls
    plain_cache = m.cache_build(support, n_groups=2)
    k0, v0 = plain_cache.get()
    same_cache = m.cache_build(support, n_groups=2, lengths=full6)
    assert np.array_equal(same_cache.counts(), [3 * T, 3 * T]) and np.array_equal(plain_cache.counts(), [3 * T, 3 * T])
    assert _same(same_cache.get()[0], k0) and np.array_equal(same_cache.get()[1], v0)
    plain = m.cache_score(plain_cache, query, THETAS, LAMBDAS, group=group, **ALL)
    again = m.cache_score(same_cache, query, THETAS, LAMBDAS, group=group, lengths=full5, **ALL)
    plain_self = m.cache_self_score(query, THETAS, LAMBDAS, 4, cache=plain_cache, group=group, **ALL)
    again_self = m.cache_self_score(query, THETAS, LAMBDAS, 4, cache=same_cache, group=group, lengths=full5, **ALL)
    for key in ALL:
        assert _same(again[key], plain[key]) and _same(again_self[key], plain_self[key]), key
    SC = dict(logprob=True, rank=True, entropy=True, argmax=True, row_nll=True)
    s_plain = m.score(query, **SC)
    s_full = m.score(query, lengths=full5, **SC)
    for key in SC:
        assert _same(s_full[key], s_plain[key]), key
    same_cache.close()

    # ---- law 3: the entries, at every pass size, against the unmasked build with the same pass size
    rng = np.random.RandomState(17)
    support2, query2 = MR.scramble_padding(support, sl, V, rng), MR.scramble_padding(query, ql, V, rng)
    assert not np.array_equal(support, support2) and not np.array_equal(query, query2)
    ragged = None
    for P in (0, 3, 4):
        whole = m.cache_build(support, n_groups=2, pass_rows=P)
        kf, vf = whole.get()
        whole.close()
        for sup in (support, support2):                                     # law 2: the padding tokens change no bit of the cache
            built = m.cache_build(sup, n_groups=2, pass_rows=P, lengths=sl)
            assert np.array_equal(built.counts(), counts) and built.info()['entries'] == 3 * T
            k, v = built.get()
            for g in range(2):
                kept = CL.scored(sl[3 * g:3 * g + 3], T).reshape(-1)
                n = counts[g]
                assert _same(k[g, :n], kf[g][kept]) and np.array_equal(v[g, :n], vf[g][kept]), (P, g)
                assert not k[g, n:].any() and not v[g, n:].any(), (P, g)
            if P == 0 and sup is support:
                ragged = built
            else:
                built.close()
    k, v = ragged.get()
    trimmed = _trimmed(m, k, v, counts)

    # ---- score_masked: law 5 against score, law 2
    s_m = m.score(query, lengths=ql, **SC)
    for key in ('logprob', 'rank', 'entropy', 'argmax'):
        assert _same(s_m[key][keep], s_plain[key][keep]) and not s_m[key][~keep].any(), key
    assert _same(s_m['row_nll'], CL.row_nll(s_m['logprob'], ql))
    s_m2 = m.score(query2, lengths=ql, **SC)
    for key in SC:
        assert _same(s_m2[key], s_m[key]), key
    win = m.score(query, lengths=ql, nll_first=2, nll_count=5, logprob=True, row_nll=True)
    assert _same(win['row_nll'], CL.row_nll(s_m['logprob'], ql, 2, 5)) and np.isnan(win['row_nll'][1]) and np.isnan(win['row_nll'][4])
    assert np.isfinite(win['row_nll'][[0, 2, 3]]).all()

    # ---- cache_score_masked / cache_self_score_masked against the ragged cache: laws 5, 2 and 4, pass sizes
    unmasked = m.cache_score(ragged, query, THETAS, LAMBDAS, group=group, **ALL)
    masked = m.cache_score(ragged, query, THETAS, LAMBDAS, group=group, lengths=ql, **ALL)
    _prefix('score', masked, unmasked, keep, ql)
    unmasked_self = m.cache_self_score(query, THETAS, LAMBDAS, 4, cache=ragged, group=group, **ALL)
    masked_self = m.cache_self_score(query, THETAS, LAMBDAS, 4, cache=ragged, group=group, lengths=ql, **ALL)
    _prefix('self', masked_self, unmasked_self, keep, ql)
    for k_ in range(3):
        assert _same(masked['logprob'][k_, 0], masked['lstm_logprob'])      # lambda = 0: the model's log-prob bitwise
        assert _same(masked_self['logprob'][k_, 0], masked_self['lstm_logprob'])
    assert _same(masked['lstm_logprob'], s_m['logprob'])
    for key in ALL:                                                         # law 2
        assert _same(m.cache_score(ragged, query2, THETAS, LAMBDAS, group=group, lengths=ql, **ALL)[key], masked[key]), key
        assert _same(m.cache_self_score(query2, THETAS, LAMBDAS, 4, cache=ragged, group=group, lengths=ql, **ALL)[key],
                     masked_self[key]), key
    for g in range(2):                                                      # law 4: rows of one group, on the trimmed copy
        sel = np.flatnonzero(group == g)
        one = m.cache_score(trimmed[g], query[sel], THETAS, LAMBDAS, pass_rows=5, **ALL)
        whole = m.cache_score(ragged, query[sel], THETAS, LAMBDAS, group=group[sel], pass_rows=5, **ALL)
        one_s = m.cache_self_score(query[sel], THETAS, LAMBDAS, 4, cache=trimmed[g], **ALL)
        whole_s = m.cache_self_score(query[sel], THETAS, LAMBDAS, 4, cache=ragged, group=group[sel], **ALL)
        for key in ALL:
            assert _same(one[key], whole[key]) and _same(one_s[key], whole_s[key]), (g, key)
    for P in (3, 4):                                                        # passes: the pieces scored in calls of their own
        p = m.cache_score(ragged, query, THETAS, LAMBDAS, group=group, lengths=ql, pass_rows=P, nll_first=1, nll_count=6, **ALL)
        u = m.cache_score(ragged, query, THETAS, LAMBDAS, group=group, pass_rows=P, **ALL)
        _prefix('pass %d' % P, p, u, keep, ql, 1, 6)
        a = m.cache_score(ragged, query[:P], THETAS, LAMBDAS, group=group[:P], lengths=ql[:P], nll_first=1, nll_count=6, **ALL)
        b = m.cache_score(ragged, query[P:], THETAS, LAMBDAS, group=group[P:], lengths=ql[P:], nll_first=1, nll_count=6, **ALL)
        for key, axis in (('logprob', 2), ('cache_prob', 1), ('lstm_logprob', 0), ('row_nll', 2)):
            assert _same(p[key], np.concatenate([a[key], b[key]], axis=axis)), (P, key)
    only = m.cache_score(ragged, query, THETAS, LAMBDAS, group=group, lengths=ql, logprob=False, cache_prob=True, row_nll=False)
    assert set(only) == {'cache_prob'} and _same(only['cache_prob'], masked['cache_prob'])

    # ---- the fp64 oracle over the trimmed entries, masked to the scored positions: test_score_against_the_fp64_oracle's bounds
    oracle = _oracle(name)
    ref0 = CL.score(oracle, 2, sl, ql, group, [1.0], [0.0])
    keys64, hq = ref0['keys'], ref0['queries']
    assert np.array_equal(ref0['counts'], counts)
    dmax = max(float(np.abs(hq[r].dot(keys64[group[r]][:counts[group[r]]].T)).max()) for r in range(5))
    thetas = [0.3 / dmax, 5.0 / dmax, 40.0 / dmax]
    want = CL.score(oracle, 2, sl, ql, group, thetas, LAMBDAS)
    got = m.cache_score(ragged, query, thetas, LAMBDAS, group=group, lengths=ql, **ALL)
    l1 = np.array([[np.abs(hq[r, t]).sum() + np.abs(keys64[group[r]]).sum(axis=1).max() for t in range(T)] for r in range(5)])
    e_lstm = float(np.abs(got['lstm_logprob'] - want['lstm_logprob']).max())
    print('%s %s: LSTM log-prob error %.3g' % (name, lens, e_lstm))
    assert e_lstm <= 1e-4
    for k_, th in enumerate(thetas):
        bound = 1e-4 + th * 2e-5 * l1
        for j, lam in enumerate(LAMBDAS):
            w, g_ = want['logprob'][k_, j], got['logprob'][k_, j].astype(np.float64)
            fin = np.isfinite(w)
            assert np.array_equal(g_[~fin], w[~fin])
            err = np.abs(g_[fin] - w[fin])
            print('%s %s theta %.3g lambda %.2f: log-prob error %.3g (bound %.3g .. %.3g)' % (name, lens, th, lam, err.max(), bound.min(), bound.max()))
            assert np.all(err <= bound[fin]), (k_, j)
            assert not g_[~keep].any()
        fin = np.isfinite(want['row_nll'][k_])
        assert np.array_equal(got['row_nll'][k_][~fin], want['row_nll'][k_][~fin])
        assert np.all(np.abs(got['row_nll'][k_][fin] - want['row_nll'][k_][fin]) <= float(bound.max()))

    # ---- eval: the fp64 storage-order sum of cache_score_masked's log-probs, bitwise; lambda = 0 against the restatement
    sup3, qry3, sl3, ql3 = support.reshape(2, 3, T), query[:4].reshape(2, 2, T), sl.reshape(2, 3), ql[:4].reshape(2, 2)
    grp4 = np.array([0, 0, 1, 1], np.int32)
    for theta, lam in ((2.0, 0.25), (9.0, 0.0)):
        lp = m.cache_score(ragged, query[:4], [theta], [lam], group=grp4, lengths=ql[:4], row_nll=False)['logprob'].reshape(4, T)
        total = 0.0
        for r in range(4):
            for t in range(int(ql[r])):
                total += float(lp[r, t])
        want_nll = np.float32(-total / int(ql[:4].sum()))
        got_nll = m.cache_eval_step(sup3, qry3, theta, lam, support_len=sl3, query_len=ql3)
        assert got_nll == want_nll, (theta, lam)
        assert m.cache_eval_step(MR.scramble_padding(sup3, sl3, V, rng), MR.scramble_padding(qry3, ql3, V, rng), theta, lam,
                                 support_len=sl3, query_len=ql3) == got_nll                      # law 2
    ref_nll = -float(oracle['lp'][:4][keep[:4]].sum()) / int(ql[:4].sum())
    zero = m.cache_eval_step(sup3, qry3, 9.0, 0.0, support_len=sl3, query_len=ql3)
    base = m.eval_step_masked(qry3, ql3)
    print('%s %s: lambda 0 NLL %.6f, eval_step_masked %.6f, fp64 %.6f' % (name, lens, zero, base, ref_nll))
    assert abs(zero - ref_nll) <= 1e-4 and abs(base - ref_nll) <= 1e-4
    full_eval = m.cache_eval_step(sup3, qry3, 2.0, 0.25, support_len=np.full((2, 3), T), query_len=np.full((2, 2), T))
    assert full_eval == m.cache_eval_step(sup3, qry3, 2.0, 0.25)                                 # law 1
    _close(trimmed + [ragged, plain_cache])


# ------------------------------------------------------------------------------------------------ generation
def test_generation_from_a_masked_built_cache():
    cfg, m, _ = _shape('H24')
    support, _, _ = _episode_rows(cfg)
    sl = np.array(SUPPORT_LENS['16+30'], np.int32)
    ragged = m.cache_build(support, n_groups=2, lengths=sl)
    counts = ragged.counts()
    k, v = ragged.get()
    trimmed = _trimmed(m, k, v, counts)
    group = np.array([0, 1, 1, 0], np.int32)
    kw = dict(temperature=1.0, seed=5, logprobs=True)
    toks, lp = m.cache_generate(ragged, 4, 6, 4.0, 0.5, group=group, **kw)
    t2, lp2 = m.cache_generate(ragged, 4, 6, 4.0, 0.5, group=group, **kw)
    assert np.array_equal(toks, t2) and _same(lp, lp2)                      # two identical calls
    stoks, slp = m.cache_self_generate(4, 6, 4.0, 0.5, 3, cache=ragged, group=group, **kw)
    s2, slp2 = m.cache_self_generate(4, 6, 4.0, 0.5, 3, cache=ragged, group=group, **kw)
    assert np.array_equal(stoks, s2) and _same(slp, slp2)
    for g in range(2):                                                      # law 4: the same four rows, all on the trimmed copy
        sel = group == g
        wt, wl = m.cache_generate(trimmed[g], 4, 6, 4.0, 0.5, **kw)
        assert np.array_equal(toks[sel], wt[sel]) and _same(lp[sel], wl[sel]), g
        wt, wl = m.cache_self_generate(4, 6, 4.0, 0.5, 3, cache=trimmed[g], **kw)
        assert np.array_equal(stoks[sel], wt[sel]) and _same(slp[sel], wl[sel]), g
    _close(trimmed + [ragged])


# ------------------------------------------------------------------------------------------------ errors, alternation
def test_refusals_touch_nothing_and_calls_alternate_freely():
    from fsmg import binding as B
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m, m2 = new_model(cfg), new_model(cfg)
    lib, T = m._lib, 8
    rng = np.random.RandomState(2)
    songs = rng.randint(0, 50, size=(4, T)).astype(np.int32)
    lens = np.array([8, 1, 5, 3], np.int32)
    I32P, F32P = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    tp = C.c_void_p(songs.ctypes.data)
    SENT = np.float32(-77.0)

    def ip(a):
        return None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(I32P)

    cache = m.cache_build(songs, n_groups=2, lengths=lens)
    foreign = m2.cache_build(songs, n_groups=2, lengths=lens)
    before = (m.score(songs)['logprob'], m.cache_score(cache, songs, [1.0], [0.5], group=[0, 0, 1, 1])['logprob'], cache.get())
    for bad in ([0, 1, 5, 3], [8, 9, 5, 3], None):
        out = np.full((4, T), SENT, np.float32)
        sc = m.score_config(4)
        assert lib.fsmg_score_masked(m._h, C.byref(sc), tp, ip(bad), out.ctypes.data_as(F32P), None, None, None, None) == -1
        assert np.all(out == SENT)
        cc = B.FsmgCacheConfig(version=B.FSMG_CACHE_CONFIG_VERSION, n_rows=4, n_groups=2)
        made = C.c_void_p()
        assert lib.fsmg_cache_build_masked(m._h, C.byref(cc), tp, ip(bad), C.byref(made)) == -1 and not made.value
        csc = m.cache_score_config(4, [1.0], [0.5])
        assert lib.fsmg_cache_score_masked(m._h, cache._c, C.byref(csc), tp, ip(bad), None, out.ctypes.data_as(F32P), None, None, None) == -1
        ssc = m.cache_self_config(3)
        assert lib.fsmg_cache_self_score_masked(m._h, cache._c, C.byref(csc), C.byref(ssc), tp, ip(bad), None, out.ctypes.data_as(F32P),
                                                None, None, None) == -1
        assert np.all(out == SENT)
        nll = C.c_float(-77.0)
        assert lib.fsmg_cache_eval_step_masked(m._h, tp, tp, ip(bad), ip(lens), 2, 2, 2, 1.0, 0.5, C.byref(nll)) == -1
        assert lib.fsmg_cache_eval_step_masked(m._h, tp, tp, ip(lens), ip(bad), 2, 2, 2, 1.0, 0.5, C.byref(nll)) == -1
        assert nll.value == -77.0
    keys, vals = np.zeros((2, 4, 16), np.float32), np.zeros((2, 4), np.int32)
    for bad in ([0, 4], [1, 5], None):
        made = C.c_void_p()
        assert lib.fsmg_cache_create_from_counts(m._h, 2, 4, ip(bad), keys.ctypes.data_as(F32P), ip(vals), C.byref(made)) == -1
        assert not made.value
    vals_bad = vals.copy()
    vals_bad[0, 0] = 52                                                     # inside the count: refused; behind it: not read
    with pytest.raises(B.FsmgError) as e:
        m.cache_from(keys, vals_bad, counts=[1, 4])
    assert e.value.code == -7
    vals_bad[0, 0], vals_bad[0, 1] = 0, 52
    keys_nan = keys.copy()
    keys_nan[0, 1:] = np.nan
    ok = m.cache_from(keys_nan, vals_bad, counts=[1, 4])
    assert not ok.get()[0].any() and not ok.get()[1].any()
    ok.close()
    cnt = np.full(2, -5, np.int32)
    assert lib.fsmg_cache_counts(m._h, foreign._c, ip(cnt)) == -1           # a foreign cache: an error, not a crash
    assert lib.fsmg_cache_counts(m._h, cache._c, None) == -1
    csc = m.cache_score_config(4, [1.0], [0.5])
    out = np.full((4, T), SENT, np.float32)
    assert lib.fsmg_cache_score_masked(m._h, foreign._c, C.byref(csc), tp, ip(lens), None, out.ctypes.data_as(F32P), None, None, None) == -1
    assert np.all(out == SENT)
    with pytest.raises(ValueError):
        m.score(songs, lengths=[8, 1, 5])                                   # the binding's own check
    # nothing was touched, and masked and unmasked calls alternate freely: the existing calls keep their bits in between
    for _ in range(2):
        assert _same(m.score(songs)['logprob'], before[0])
        masked = m.score(songs, lengths=lens)['logprob']
        assert _same(masked[CL.scored(lens, T)], before[0][CL.scored(lens, T)])
        assert _same(m.cache_score(cache, songs, [1.0], [0.5], group=[0, 0, 1, 1])['logprob'], before[1])
        m.cache_score(cache, songs, [1.0], [0.5], group=[0, 0, 1, 1], lengths=lens)
        uniform = m.cache_build(songs, n_groups=2)
        assert np.array_equal(uniform.counts(), [2 * T, 2 * T])
        uniform.close()
        again = m.cache_build(songs, n_groups=2, lengths=lens)
        assert _same(again.get()[0], before[2][0]) and np.array_equal(again.get()[1], before[2][1])
        again.close()
        m.cache_eval_step(songs.reshape(2, 2, T), songs.reshape(2, 2, T), 1.0, 0.5, support_len=lens.reshape(2, 2), query_len=lens.reshape(2, 2))
    assert np.array_equal(cache.counts(), [9, 8])
    foreign.close()
    cache.close()
    m2.close()


# ------------------------------------------------------------------------------------------------ the plugin
class _Episode(object):
    def __init__(self, support, query, support_len=None, query_len=None):
        self.support, self.query, self.support_len, self.query_len = support, query, support_len, query_len


def test_plugin_with_cache_lengths(tmp_path):
    from models.cache_lstm import CacheLSTM
    cfg = dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name='cache_masked_lstm',
               checkpt_dir=str(tmp_path / 'cache'), cache_theta=1.5, cache_lambda=0.25, cache_lengths=True)
    model = CacheLSTM(cfg)
    model.recover_or_init('')
    rng = np.random.RandomState(5)
    episodes = []
    for _ in range(2):
        support = rng.randint(0, 40, size=(3, 2, 12)).astype(np.int32)
        query = rng.randint(0, 40, size=(3, 4, 12)).astype(np.int32)
        query[:, 0] = support[:, 1]
        episodes.append(_Episode(support, query, MR.lengths_for(rng, (3, 2), 12), MR.lengths_for(rng, (3, 4), 12)))
    for e in episodes:
        model.train(e)                                                      # training is the baseline's unmasked step
    ep = episodes[0]
    m = model.engine
    want = m.cache_eval_step(ep.support, ep.query, 1.5, 0.25, support_len=ep.support_len, query_len=ep.query_len)
    assert model.eval(ep) == want
    assert want != m.cache_eval_step(ep.support, ep.query, 1.5, 0.25)       # and the lengths do something
    assert model.eval_many(episodes) == [model.eval(e) for e in episodes]
    thetas, lambdas = [0.0, 1.5], [0.0, 0.25, 0.5]
    grid = model.tune(episodes, thetas, lambdas)
    assert grid.shape == (2, 3)
    for k, th in enumerate(thetas):
        for j, lam in enumerate(lambdas):
            one = np.mean([m.cache_eval_step(e.support, e.query, th, lam, support_len=e.support_len, query_len=e.query_len) for e in episodes])
            assert abs(grid[k, j] - one) <= 1e-5 * max(1.0, abs(one)), (k, j)
    songs, lens = ep.query.reshape(-1, 12), ep.query_len.reshape(-1)
    got = model.score(ep.support, songs, support_lengths=ep.support_len.reshape(-1), lengths=lens, cache_prob=True)
    cache = m.cache_build(ep.support.reshape(-1, 12), n_groups=1, lengths=ep.support_len.reshape(-1))
    ref = m.cache_score(cache, songs, [1.5], [0.25], lengths=lens, cache_prob=True)
    assert np.array_equal(cache.counts(), [ep.support_len.sum()])
    cache.close()
    for key in ('logprob', 'cache_prob', 'row_nll'):
        assert _same(got[key], ref[key]), key
    with pytest.raises(ValueError, match='no support_len'):
        model.eval(_Episode(ep.support, ep.query))
    with pytest.raises(ValueError, match='needs support_lengths'):
        model.score(ep.support, songs)
    own = model.score_self(songs, lengths=lens)
    assert _same(own['logprob'], m.cache_self_score(songs, 1.5, 0.25, 12, lengths=lens)['logprob'])
    with pytest.raises(ValueError, match='needs support_len'):
        model.generate(ep.support[0], 5, n=2, cache=True, temperature=1.0)
    out = model.generate(ep.support[0], 5, n=2, cache=True, support_len=ep.support_len[0], temperature=1.0, seed=3)
    assert len(out) == 2
    with pytest.raises(RuntimeError, match='CacheLSTM has no padding-masked loss'):
        CacheLSTM(dict(cfg, mask_padding=True, checkpt_dir=str(tmp_path / 'refused')))
