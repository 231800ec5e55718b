"""The support-set neural cache (fsmg_cache_*) on the MI355X against the fp64 numpy restatement of its contract (tests/cache_ref.py):
the attention kernel at tile edges, the build against fsmg_score's own hidden states, scoring against the GPU's own vectors and
against the fp64 oracle, eval and the plugin, side effects, errors.

Tolerances of the attention tests come from the reference, inside the test: e32 is the error of the restatement evaluated in fp32
against fp64 on the same fp32 inputs, and the GPU must be within max(8 * e32, 1e-6) -- relative for p_cache > 0 (the margin of 8
covers a summation order the restatement does not share)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cache_ref as R
import score_ref as S
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O
from test_score import SHAPES as SCORE_SHAPES

pytestmark = pytest.mark.gpu

SHAPES = {k: SCORE_SHAPES[k][0] for k in ('H24', 'H200x2', 'H512', 'H1024x2')}
N_TOKENS = 7                    # the attention tests draw values from 7 tokens: every target has several hits; 7 itself occurs nowhere


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, want64):
    """max relative error over want > 0; where want == 0 the result must be exactly 0"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    pos = want64 > 0
    assert np.all(got[~pos] == 0.0), 'a target no entry holds must give exactly 0'
    return float((np.abs(got[pos] - want64[pos]) / want64[pos]).max()) if pos.any() else 0.0


def _check_attend(tag, got, keys, vals, q, y, group, thetas):
    """got against fp64 within max(8 * e32, 1e-6), e32 the fp32 restatement's own error on the same inputs; -> (e32, error)"""
    p64 = R.attend_groups(keys, vals, q, y, group, thetas)
    p32 = R.attend_groups(keys, vals, q, y, group, thetas, np.float32)
    e32, err = _rel_err(p32, p64), _rel_err(got, p64)
    print('%s: e32 %.3g, GPU %.3g' % (tag, e32, err))
    assert err <= max(8 * e32, 1e-6), tag
    return e32, err


@functools.lru_cache(maxsize=None)
def _attend_model(H):
    return new_model(small_config(input_size=20, max_len=4, embedding_size=8, hidden_size=H))


def _thetas_for(keys, q):
    """theta (d_max - d_min) about 0, about 5 and about 40 for the typical query; fp32 numbers, so that the library (whose thetas are
    floats) and both modes of the restatement see the same inputs"""
    d = q.astype(np.float64).dot(keys.reshape(-1, keys.shape[-1]).astype(np.float64).T)
    spread = float(np.median(d.max(axis=1) - d.min(axis=1)))
    spread = spread if spread > 0 else float(np.abs(d).max())
    return [0.0, float(np.float32(5.0 / spread)), float(np.float32(40.0 / spread))]


# ------------------------------------------------------------------------------------------------ 1. attend at tile edges
@pytest.mark.parametrize('H', [24, 200, 512])
def test_attend_known_answers_at_tile_edges(H):
    m = _attend_model(H)
    worst = (0.0, 0.0)
    for Mg in (1, 15, 16, 17, 63, 64, 65, 257):
        for n in (1, 17, 33):
            rng = np.random.RandomState(1000 * Mg + n)
            keys = (rng.normal(size=(1, Mg, H)) / np.sqrt(H)).astype(np.float32)
            vals = rng.randint(0, N_TOKENS, size=(1, Mg)).astype(np.int32)
            q = rng.normal(size=(n, H)).astype(np.float32) * 3
            y = rng.randint(0, N_TOKENS + 1, size=n).astype(np.int32)
            y[0] = vals[0, 0]                                  # at least one hit ...
            if n > 1:
                y[1] = N_TOKENS                                # ... and one target that occurs nowhere
            thetas = _thetas_for(keys, q)
            cache = m.cache_from(keys, vals)
            got = m.cache_attend(cache, q, y, thetas)
            assert got.shape == (3, n) and got.dtype == np.float32
            assert _same(got, m.cache_attend(cache, q, y, thetas))          # two identical calls: identical bits
            cache.close()
            pair = _check_attend('H %d Mg %d n %d' % (H, Mg, n), got, keys, vals, q, y, None, thetas)
            worst = max(worst, pair, key=lambda p: p[1])
            assert np.all(got[:, y == N_TOKENS] == 0.0)
            if Mg == 1:
                assert np.all(got[:, y == vals[0, 0]] == 1.0)               # one entry: all the mass or none
    print('H %d: largest GPU error %.3g (e32 there %.3g)' % (H, worst[1], worst[0]))


@pytest.mark.parametrize('H', [24, 200, 512])
def test_attend_all_scores_negative_masks_the_tail(H):
    """keys = -|.| against queries = +|.| with theta d <= -5: a pad key scored as zero would take nearly all the mass"""
    m = _attend_model(H)
    for Mg in (1, 15, 17, 63, 65, 257):
        rng = np.random.RandomState(Mg)
        keys = (-np.abs(rng.normal(size=(1, Mg, H))) / np.sqrt(H)).astype(np.float32)
        vals = rng.randint(0, N_TOKENS, size=(1, Mg)).astype(np.int32)
        q = np.abs(rng.normal(size=(17, H))).astype(np.float32)
        y = vals[0, rng.randint(0, Mg, size=17)].astype(np.int32)          # every target has a hit
        d = q.astype(np.float64).dot(keys[0].astype(np.float64).T)
        assert d.max() < 0
        theta = float(np.float32(5.001 / -d.max()))                        # an fp32 number (2 * theta is one too) with theta d <= -5
        cache = m.cache_from(keys, vals)
        got = m.cache_attend(cache, q, y, [theta, 2 * theta])
        cache.close()
        _check_attend('negative H %d Mg %d' % (H, Mg), got, keys, vals, q, y, None, [theta, 2 * theta])
        assert np.all(got > 0)
        if Mg == 1:
            assert np.all(got == 1.0)


@pytest.mark.parametrize('H', [24, 512])
def test_attend_group_isolation_and_row_independence(H):
    m = _attend_model(H)
    rng = np.random.RandomState(3)
    Mg, n = 65, 33
    keys = (rng.normal(size=(2, Mg, H)) / np.sqrt(H)).astype(np.float32)
    vals = rng.randint(0, N_TOKENS, size=(2, Mg)).astype(np.int32)
    q = rng.normal(size=(n, H)).astype(np.float32) * 3
    y = rng.randint(0, N_TOKENS, size=n).astype(np.int32)
    thetas = _thetas_for(keys[:1], q)
    one = m.cache_from(keys[:1], vals[:1])
    base = m.cache_attend(one, q, y, thetas)
    # in the OTHER group: a key equal to 50 x the query, holding the query's target -- it must not be seen
    for i in range(min(n, Mg)):
        keys[1, i], vals[1, i] = 50.0 * q[i], y[i]
    two = m.cache_from(keys, vals)
    assert _same(base, m.cache_attend(two, q, y, thetas, group=np.zeros(n, np.int32)))
    assert _same(base, m.cache_attend(two, q, y, thetas))                   # group NULL = all 0
    # mixed groups: every query's bits are those of its own group's call
    group = rng.randint(0, 2, size=n).astype(np.int32)
    mixed = m.cache_attend(two, q, y, thetas, group=group)
    other = m.cache_attend(two, q, y, thetas, group=np.ones(n, np.int32))
    assert _same(mixed, np.where(group[None, :] == 0, base, other))
    assert np.all(other[1:, :min(n, Mg)] > 0.99)                             # there the planted key IS seen
    _check_attend('two groups H %d' % H, mixed, keys, vals, q, y, group, thetas)
    # permuting the queries permutes the outputs bitwise; a query alone gives the bits it gives among 32 others
    perm = rng.permutation(n)
    assert _same(m.cache_attend(two, q[perm], y[perm], thetas, group=group[perm]), mixed[:, perm])
    for i in (0, 16, 32):
        assert _same(m.cache_attend(two, q[i:i + 1], y[i:i + 1], thetas, group=group[i:i + 1]), mixed[:, i:i + 1])
    assert one.info() == dict(groups=1, entries=Mg, hidden=H, bytes=one.info()['bytes']) and one.info()['bytes'] >= Mg * (H + 1) * 4
    one.close()
    two.close()


# ------------------------------------------------------------------------------------------------ shared: one trained model per shape
def _trained(cfg, steps=3, seed=7, **kw):
    m = new_model(cfg, **kw)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


def _songs(cfg, rows, seed=0):
    return np.random.RandomState(seed).randint(0, cfg['input_size'], size=(rows, cfg['max_len'])).astype(np.int32)


def _episode_rows(cfg):
    """6 support rows in 2 groups; 5 query rows: row 0 a copy of a support row of its own group, row 1 sharing that row's first half"""
    support = _songs(cfg, 6, seed=11)
    query = _songs(cfg, 5, seed=12)
    group = np.array([0, 0, 1, 1, 0], np.int32)
    query[0] = support[1]
    query[1, :cfg['max_len'] // 2] = support[1, :cfg['max_len'] // 2]
    return support, query, group


@functools.lru_cache(maxsize=None)
def _shape(name):
    """One model per shape with the ORACLE's parameters: its initialiser and three of its train steps, uploaded.  The copied-row
    property of test_score_against_the_fp64_oracle is a property of the reference on these parameters and rows: computed with the
    oracle alone (no GPU), the copied row gains 1.46 / 0.37 / 0.43 / 1.01 nats at the sharpest theta at H24 / H200x2 / H512 /
    H1024x2 and 0.9 nats or more at the other two.  (It is NOT a property of every parameter set: on the library's own initialiser
    and three GPU train steps the reference itself loses 0.045 nats at H200x2 at the sharpest theta -- the largest dot product is
    then a late, long key, not the query's own.)  -> (cfg, model, the uploaded parameters in fp64)"""
    cfg = small_config(**SHAPES[name])
    params = O.glorot_init(cfg, cfg['seed'])
    opt = O.new_opt_state(params)
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=7):
        O.train_step(params, opt, sup, qry, cfg)
    m = new_model(cfg, params=params)
    return cfg, m, f64_params(m)


def _top_hidden(m, cfg, rows):
    """the top-layer hidden states of the last pass (over `rows` rows) as [rows, T, H], and the pad units"""
    d = m.debug_dims()
    T, Hp, H = d['T'], d['Hp'], cfg['hidden_size']
    hs = m.debug_read('h%d' % (cfg['n_layers'] - 1), (T + 1) * rows * Hp).reshape(T + 1, rows, Hp)[1:]
    return np.ascontiguousarray(hs[:, :, :H].transpose(1, 0, 2)), hs[:, :, H:]


# ------------------------------------------------------------------------------------------------ 2. build
@pytest.mark.parametrize('name', list(SHAPES))
def test_build_files_fsmg_scores_hidden_states(name):
    cfg, m, _ = _shape(name)
    support, query, group = _episode_rows(cfg)
    T, H = cfg['max_len'], cfg['hidden_size']
    cache = m.cache_build(support.reshape(2, 3, T), n_groups=2)
    assert cache.info()['groups'] == 2 and cache.info()['entries'] == 3 * T and cache.info()['hidden'] == H
    keys, vals = cache.get()
    m.score(support)
    hs, pad = _top_hidden(m, cfg, 6)
    assert np.all(pad == 0)                                                 # the pad units are exact zeros
    assert _same(keys.reshape(6, T, H), hs)                                 # bitwise fsmg_score's hidden states
    assert np.array_equal(vals.reshape(6, T), support)
    # get -> cache_from -> attend: the same bits as the built cache
    q = hs.reshape(6 * T, H)[::5]
    y = support.reshape(-1)[::5]
    g = (np.arange(6 * T)[::5] // (3 * T)).astype(np.int32)
    thetas = [0.0, 1.0, 6.0]
    copy = m.cache_from(keys, vals)
    built = m.cache_attend(cache, q, y, thetas, group=g)
    assert _same(built, m.cache_attend(copy, q, y, thetas, group=g))
    assert np.all(built > 0)                                                # every query is one of its group's own keys
    copy.close()
    # passes: the cache is bitwise what building each pass's rows in a call of their own gives
    for P, parts in ((3, ((0, 3), (3, 6))), (4, ((0, 4), (4, 6)))):
        whole = m.cache_build(support, n_groups=2, pass_rows=P)
        k2, v2 = whole.get()
        pieces = [m.cache_build(support[a:b], n_groups=1) for a, b in parts]
        assert _same(k2.reshape(6, T, H), np.concatenate([p.get()[0].reshape(-1, T, H) for p in pieces])), P
        assert np.array_equal(v2.reshape(6, T), support)
        for c in pieces + [whole]:
            c.close()
    again = m.cache_build(support, n_groups=2)
    assert _same(again.get()[0], keys)                                      # two identical calls: identical bits
    again.close()
    cache.close()


# ------------------------------------------------------------------------------------------------ 3. score against the GPU's own vectors
def _ulp_close(got, want32):
    got, want32 = np.asarray(got, np.float32), np.asarray(want32, np.float32)
    fin = np.isfinite(want32)
    return np.array_equal(got[~fin], want32[~fin]) and np.all(np.abs(got[fin].astype(np.float64) - want32[fin]) <= np.spacing(np.abs(want32[fin])))


@pytest.mark.parametrize('name', list(SHAPES))
def test_score_against_the_gpus_own_vectors(name):
    cfg, m, _ = _shape(name)
    support, query, group = _episode_rows(cfg)
    T = cfg['max_len']
    thetas, lambdas = [0.0, 2.0, 9.0], [0.0, 0.25, 1.0]
    cache = m.cache_build(support, n_groups=2)
    ALL = dict(logprob=True, cache_prob=True, lstm_logprob=True, row_nll=True)
    got = m.cache_score(cache, query, thetas, lambdas, group=group, **ALL)
    assert got['logprob'].shape == (3, 3, 5, T) and got['cache_prob'].shape == (3, 5, T) and got['row_nll'].shape == (3, 3, 5)
    hq, _ = _top_hidden(m, cfg, 5)
    assert _same(got['lstm_logprob'], m.score(query)['logprob'])
    want_pc = m.cache_attend(cache, hq.reshape(5 * T, -1), query.reshape(-1), thetas, group=np.repeat(group, T))
    assert _same(got['cache_prob'], want_pc.reshape(3, 5, T))
    for k in range(3):
        for j, lam in enumerate(lambdas):
            assert _ulp_close(got['logprob'][k, j], R.mix(got['lstm_logprob'], got['cache_prob'][k], lam)), (k, j)
            assert _same(got['row_nll'][k, j], S.row_nll(got['logprob'][k, j]))
        assert _same(got['logprob'][k, 0], got['lstm_logprob'])             # lambda = 0: the model's log-prob bitwise
    assert _same(got['logprob'], m.cache_score(cache, query, thetas, lambdas, group=group)['logprob'])   # the same call twice
    # windows and NULL outputs keep the other outputs' bits
    win = m.cache_score(cache, query, thetas, lambdas, group=group, nll_first=4, nll_count=5, **ALL)
    for k in range(3):
        for j in range(3):
            assert _same(win['row_nll'][k, j], S.row_nll(got['logprob'][k, j], 4, 5))
    for key in ALL:
        only = m.cache_score(cache, query, thetas, lambdas, group=group, nll_first=4, nll_count=5, **{k: k == key for k in ALL})
        assert set(only) == {key} and _same(only[key], win[key]), key
    # passes: rows 3 at a time are the bits of the pieces scored in calls of their own
    p3 = m.cache_score(cache, query, thetas, lambdas, group=group, pass_rows=3, **ALL)
    a = m.cache_score(cache, query[:3], thetas, lambdas, group=group[:3], **ALL)
    b = m.cache_score(cache, query[3:], thetas, lambdas, group=group[3:], **ALL)
    for key, axis in (('logprob', 2), ('cache_prob', 1), ('lstm_logprob', 0), ('row_nll', 2)):
        assert _same(p3[key], np.concatenate([a[key], b[key]], axis=axis)), key
    cache.close()


# ------------------------------------------------------------------------------------------------ 4. score against the fp64 oracle
@pytest.mark.parametrize('name', list(SHAPES))
def test_score_against_the_fp64_oracle(name):
    cfg, m, params = _shape(name)
    support, query, group = _episode_rows(cfg)
    T = cfg['max_len']
    lambdas = [0.0, 0.25, 1.0]
    ref0 = R.score(params, support, 2, query, group, [1.0], [0.0], cfg)
    keys, hq = ref0['keys'], ref0['queries']
    dmax = max(float(np.abs(hq[r].dot(keys[group[r]].T)).max()) for r in range(5))
    thetas = [0.3 / dmax, 5.0 / dmax, 40.0 / dmax]                          # theta max|q . k| = 0.3, 5, 40, from the oracle's vectors
    want = R.score(params, support, 2, query, group, thetas, lambdas, cfg)
    cache = m.cache_build(support, n_groups=2)
    got = m.cache_score(cache, query, thetas, lambdas, group=group, cache_prob=True, lstm_logprob=True)
    cache.close()
    # what the project's 2e-5 per-unit hidden-state bound allows in a score: 2e-5 max_i sum_j (|q_j| + |k_ij|), per query
    l1 = np.array([[np.abs(hq[r, t]).sum() + np.abs(keys[group[r]]).sum(axis=1).max() for t in range(T)] for r in range(5)])
    e_lstm = float(np.abs(got['lstm_logprob'] - want['lstm_logprob']).max())
    assert e_lstm <= 1e-4
    for k, th in enumerate(thetas):
        bound = 1e-4 + th * 2e-5 * l1
        for j, lam in enumerate(lambdas):
            w, g = want['logprob'][k, j], got['logprob'][k, j].astype(np.float64)
            fin = np.isfinite(w)
            assert np.array_equal(g[~fin], w[~fin])                         # lambda = 1 where no entry holds the target: -inf
            err = np.abs(g[fin] - w[fin])
            print('%s theta %.3g lambda %.2f: log-prob error %.3g (bound %.3g .. %.3g), LSTM %.3g'
                  % (name, th, lam, err.max(), bound.min(), bound.max(), e_lstm))
            assert np.all(err <= bound[fin]), (k, j)
        fin = np.isfinite(want['row_nll'][k])
        assert np.array_equal(got['row_nll'][k][~fin], want['row_nll'][k][~fin])
        assert np.all(np.abs(got['row_nll'][k][fin] - want['row_nll'][k][fin]) <= float(bound.max()))
        # the copied row: the cache holds its own continuation at every position
        nll_mix, nll_lstm = float(got['row_nll'][k, 1, 0]), float(-got['lstm_logprob'][0].astype(np.float64).mean())
        print('%s theta %.3g: copied row %.4f mixed against %.4f LSTM' % (name, th, nll_mix, nll_lstm))
        assert nll_mix < nll_lstm


# ------------------------------------------------------------------------------------------------ 5. eval and plugin
class _Episode(object):
    def __init__(self, support, query):
        self.support, self.query = support, query


def test_eval_step_and_plugin(tmp_path):
    from models.cache_lstm import CacheLSTM
    from models.lstm_baseline import LSTMBaseline
    cfg = dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name='cache_lstm',
               checkpt_dir=str(tmp_path / 'cache'), cache_theta=1.5, cache_lambda=0.25)
    model = CacheLSTM(cfg)
    model.recover_or_init('')
    rng = np.random.RandomState(5)
    episodes = []
    for _ in range(2):
        support = rng.randint(0, 40, size=(3, 2, 12)).astype(np.int32)
        query = rng.randint(0, 40, size=(3, 4, 12)).astype(np.int32)
        query[:, 0] = support[:, 1]
        episodes.append(_Episode(support, query))
    ep = episodes[0]
    for e in episodes:
        model.train(e)
    m = model.engine
    group = np.repeat(np.arange(3), 4).astype(np.int32)
    cache = m.cache_build(ep.support, n_groups=3)
    sc = m.cache_score(cache, ep.query, [1.5], [0.25], group=group)
    cache.close()
    total = 0.0
    for v in sc['logprob'].reshape(-1):                                     # the fp64 sum in storage order, rounded once
        total += float(v)
    want = np.float32(-total / sc['logprob'].size)
    assert m.cache_eval_step(ep.support, ep.query, 1.5, 0.25) == want
    assert model.eval(ep) == want
    assert model.eval_many(episodes) == [model.eval(e) for e in episodes]
    thetas, lambdas = [0.0, 1.5, 4.0], [0.0, 0.25, 0.5, 1.0]
    grid = model.tune(episodes, thetas, lambdas)
    assert grid.shape == (3, 4)
    assert abs(grid[1, 1] - np.mean([model.eval(e) for e in episodes])) <= 1e-6
    for k, th in enumerate(thetas):
        for j, lam in enumerate(lambdas):
            one = np.mean([m.cache_eval_step(e.support, e.query, th, lam) for e in episodes])
            assert (np.isinf(one) and np.isinf(grid[k, j])) or abs(grid[k, j] - one) <= 1e-5 * max(1.0, abs(one)), (k, j)
    # lambda = 0 is the baseline
    base = LSTMBaseline.eval(model, ep)
    zero = CacheLSTM(dict(cfg, cache_lambda=0.0, checkpt_dir=str(tmp_path / 'zero')))
    zero.recover_or_init('')
    zero.engine.set_params(m.get_params())
    assert abs(zero.eval(ep) - base) <= 1e-6
    # score: one group built from the whole support set
    songs = ep.query.reshape(-1, 12)
    got = model.score(ep.support, songs, cache_prob=True)
    cache = m.cache_build(ep.support.reshape(-1, 12), n_groups=1)
    assert _same(got['logprob'], m.cache_score(cache, songs, [1.5], [0.25])['logprob'])
    cache.close()
    assert got['logprob'].shape == (1, 1, 12, 12) and got['cache_prob'].shape == (1, 12, 12)
    assert model.sample(ep.support[0], 5) == LSTMBaseline.sample(model, ep.support[0], 5)


# ------------------------------------------------------------------------------------------------ 6. side effects
def _state(m):
    return m.get_params(), {k: m.get_opt_state(k) for k in m.param_shapes}, m.step, m.read_losses(2)


def _same_state(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)), k
        assert np.array_equal(a[1][k][0], b[1][k][0]) and np.array_equal(a[1][k][1], b[1][k][1]), k
    assert a[2] == b[2] and np.array_equal(a[3], b[3])


def test_no_side_effects_stale_caches_and_separate_registries():
    from fsmg.binding import FsmgError
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    sup, qry = O.synthetic_episodes(1, 2, 2, 2, 12, 97, seed=3)[0]
    m1, m2 = _trained(cfg), _trained(cfg)
    songs = _songs(cfg, 9, seed=6)
    score0 = m1.score(songs)['logprob']
    gen0 = m1.generate(3, 12, temperature=1.0, seed=4)
    eval0 = m1.eval_step(qry)
    m1.forward_backward(sup, qry)
    m2.forward_backward(sup, qry)
    before, grads = _state(m1), {k: m1.get_grad(k) for k in m1.param_shapes}
    cache = m1.cache_build(sup, n_groups=2)
    group = np.array([0, 0, 1, 1], np.int32)
    first = m1.cache_score(cache, qry, [2.0], [0.25], group=group)
    m1.cache_eval_step(sup, qry, 2.0, 0.25)
    _same_state(before, _state(m1))
    for k, g in grads.items():
        assert np.array_equal(g.view(np.uint32), m1.get_grad(k).view(np.uint32)), k
    # the entry points that were there before return the bits they returned before a cache was built
    assert _same(score0, m1.score(songs)['logprob'])
    assert np.array_equal(gen0, m1.generate(3, 12, temperature=1.0, seed=4))
    assert eval0 == m1.eval_step(qry)
    assert m1.apply_update() == m2.apply_update()
    # after a train step the old cache still scores: stale by design (its keys are the old parameters' vectors)
    keys0 = cache.get()[0]
    assert m1.train_step(sup, qry) == m2.train_step(sup, qry)
    for k, v in m1.get_params().items():
        assert np.array_equal(v, m2.get_param(k)), k
    assert _same(cache.get()[0], keys0)
    stale = m1.cache_score(cache, qry, [2.0], [0.25], group=group)
    assert np.all(np.isfinite(stale['logprob'])) and not _same(stale['logprob'], first['logprob'])
    fresh = m1.cache_build(sup, n_groups=2)
    assert not _same(fresh.get()[0], keys0)
    # two handles keep separate registries
    other = m2.cache_build(sup, n_groups=2)
    with pytest.raises(FsmgError) as e:
        m1.cache_score(other, qry, [2.0], [0.25], group=group)
    assert e.value.code == -1
    assert m2.cache_score(other, qry, [2.0], [0.25], group=group)['logprob'].shape == (1, 1, 4, 12)
    fresh.close()
    cache.close()
    m2.close()                                                              # fsmg_destroy frees the cache still alive
    other.close()


# ------------------------------------------------------------------------------------------------ 7. errors
def test_argument_errors():
    from fsmg import binding as B
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m, m2 = new_model(cfg), new_model(cfg)
    lib = m._lib
    songs = _songs(cfg, 4)
    F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    tp = C.c_void_p(songs.ctypes.data)
    cache = m.cache_build(songs, n_groups=2)
    lp = np.empty((8, 16, 4, 8), np.float32)

    def build(tokens=tp, **over):
        c = B.FsmgCacheConfig(version=B.FSMG_CACHE_CONFIG_VERSION, n_rows=4, n_groups=2)
        for k, v in over.items():
            if k == 'reserved':
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        out = C.c_void_p()
        rc = lib.fsmg_cache_build(m._h, C.byref(c), tokens, C.byref(out))
        if rc == 0:
            assert lib.fsmg_cache_destroy(m._h, out) == 0
        return rc

    def score(handle=None, c_ptr=None, tokens=tp, group=None, out=lp, thetas=(1.0,), lambdas=(0.5,), theta0=None, lambda0=None, **over):
        c = m.cache_score_config(4, thetas, lambdas)
        for k, v in over.items():
            if k == 'reserved':
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        if theta0 is not None:
            c.thetas[0] = theta0
        if lambda0 is not None:
            c.lambdas[0] = lambda0
        g = None if group is None else np.asarray(group, np.int32)
        return lib.fsmg_cache_score((handle or m)._h, cache._c if c_ptr is None else c_ptr, C.byref(c), tokens,
                                    None if g is None else g.ctypes.data_as(I32P), None if out is None else out.ctypes.data_as(F32P),
                                    None, None, None)

    assert build() == 0 and score() == 0 and score(group=[0, 1, 1, 0]) == 0
    assert build(version=2) == -1                                           # wrong version
    assert score(version=0) == -1
    assert build(reserved=0) == -1 and build(reserved=10) == -1             # nonzero reserved
    assert score(reserved=7) == -1
    assert build(n_groups=3) == -1 and build(n_groups=0) == -1              # n_rows not a multiple of n_groups
    assert build(pass_rows=1025) == -1 and build(tokens_on_device=2) == -1 and build(tokens=None) == -1 and build(n_rows=0) == -1
    assert score(n_theta=0) == -1 and score(n_theta=9) == -1                # n_theta / n_lambda out of range
    assert score(n_lambda=0) == -1 and score(n_lambda=17) == -1
    assert score(theta0=-0.5) == -1 and score(theta0=float('nan')) == -1 and score(theta0=float('inf')) == -1
    assert score(lambda0=-0.01) == -1 and score(lambda0=1.01) == -1 and score(lambda0=float('nan')) == -1
    assert score(group=[0, 2, 0, 0]) == -1 and score(group=[0, -1, 0, 0]) == -1     # group id out of range
    assert score(out=None) == -1                                            # every output NULL
    assert score(tokens=None) == -1 and score(nll_first=8) == -1 and score(pass_rows=-1) == -1
    assert score(handle=m2) == -1                                           # another handle's cache
    assert score(thetas=[0.0] * 8, lambdas=[0.0] * 16) == 0
    q = np.zeros((2, 16), np.float32)
    y = np.zeros(2, np.int32)
    with pytest.raises(B.FsmgError) as e:
        m.cache_attend(cache, q, y, [1.0], group=[0, 2])
    assert e.value.code == -1
    with pytest.raises(B.FsmgError) as e:
        m.cache_attend(cache, q, y, [-1.0])
    assert e.value.code == -1
    with pytest.raises(ValueError):
        m.cache_attend(cache, np.zeros((2, 15), np.float32), y, [1.0])
    bad = songs.copy()                                                      # token out of range on the host path
    bad[2, 3] = 50
    for call in (lambda: m.cache_build(bad, n_groups=2), lambda: m.cache_score(cache, bad, [1.0], [0.5]),
                 lambda: m.cache_eval_step(bad.reshape(2, 2, 8), songs.reshape(2, 2, 8), 1.0, 0.5),
                 lambda: m.cache_eval_step(songs.reshape(2, 2, 8), bad.reshape(2, 2, 8), 1.0, 0.5)):
        with pytest.raises(B.FsmgError) as e:
            call()
        assert e.value.code == -7
    with pytest.raises(B.FsmgError) as e:
        m.cache_from(np.zeros((1, 2, 16), np.float32), np.array([[0, 52]], np.int32))
    assert e.value.code == -7
    for theta, lam in ((-1.0, 0.5), (1.0, 1.5)):
        with pytest.raises(B.FsmgError) as e:
            m.cache_eval_step(songs.reshape(2, 2, 8), songs.reshape(2, 2, 8), theta, lam)
        assert e.value.code == -1
    # over-limit sizes are refused before anything is read or allocated
    small_f, small_i, out = np.zeros(16, np.float32), np.zeros(4, np.int32), C.c_void_p()
    fp, ip = small_f.ctypes.data_as(F32P), small_i.ctypes.data_as(I32P)
    assert lib.fsmg_cache_create_from(m._h, 1, (1 << 22) + 1, fp, ip, C.byref(out)) == -1      # G * Mg > 2^22
    assert lib.fsmg_cache_create_from(m._h, 0, 4, fp, ip, C.byref(out)) == -1 and lib.fsmg_cache_create_from(m._h, 1, 0, fp, ip, C.byref(out)) == -1
    assert build(n_rows=1 << 20, n_groups=1) == -1                          # 2^20 rows x 8 entries > 2^22
    wide = new_model(small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=512))
    assert lib.fsmg_cache_create_from(wide._h, 1, (1 << 20) + 1, fp, ip, C.byref(out)) == -1   # keys > 2^31 bytes at Hp = 512
    with pytest.raises(B.FsmgError) as e:                                   # a cache whose H differs: another handle's, by construction
        wide.cache_attend(cache, np.zeros((1, 512), np.float32), y[:1], [1.0])
    assert e.value.code == -1
    wide.close()
    # a destroyed cache: an error, not a crash
    handle = cache._c
    cache.close()
    assert score(c_ptr=handle) == -1
    assert lib.fsmg_cache_destroy(m._h, handle) == -1 and lib.fsmg_cache_info(m._h, handle, (C.c_int64 * 4)()) == -1
    assert lib.fsmg_cache_get(m._h, handle, None, None) == -1
    with pytest.raises(B.FsmgError):
        cache.info()
    got = m.cache_build(songs, n_groups=1)                                  # the handle stays usable
    assert np.all(np.isfinite(m.cache_score(got, songs, [1.0], [0.5])['logprob']))
    got.close()
