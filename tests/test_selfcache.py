"""The self-cache (fsmg_cache_self_attend / fsmg_cache_self_score) on the MI355X against the fp64 numpy restatement of its contract
(tests/selfcache_ref.py): the causal kernel at its query-tile, key-tile and window edges, masking, bitwise independence, scoring
against the GPU's own vectors and against the fp64 oracle, the copied-half song's gain, side effects on the support-set entry points,
errors.

Tolerances.  Attention: test_cache's rule -- e32 is the error of the restatement evaluated in fp32 against fp64 on the
same fp32 inputs, and the GPU must be within max(8 * e32, 1e-6), relative where fp64 > 0, exactly 0 where fp64 is 0.  Scores against
the oracle: 1e-4 + theta * 2e-5 * l1, l1 = sum_j |q_j| + the largest sum_j |k_ij| over the entries the position sees."""
import ctypes as C
import functools

import numpy as np
import pytest

import cache_ref as R
import score_ref as S
import selfcache_ref as SC
from conftest import small_config
from gpu_utils import new_model

pytestmark = pytest.mark.gpu

N_TOKENS = 7                    # values are drawn from 7 tokens; N_TOKENS itself is planted where a target must find nothing
N_POS = (1, 2, 16, 17, 32, 33, 65)
WINDOWS = (1, 15, 16, 17, 1000)
SUPPORT = (0, 1, 17, 65)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, want64):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    pos = want64 > 0
    assert np.all(got[~pos] == 0.0), 'a target no visible entry holds must give exactly 0'
    return float((np.abs(got[pos] - want64[pos]) / want64[pos]).max()) if pos.any() else 0.0


@functools.lru_cache(maxsize=None)
def _attend_model(H):
    return new_model(small_config(input_size=20, max_len=4, embedding_size=8, hidden_size=H))


def _vectors(rng, shape):
    """dot products of two such vectors have a standard deviation of 3"""
    H = shape[-1]
    return (rng.normal(size=shape) * np.sqrt(3.0 / np.sqrt(H))).astype(np.float32)


def _thetas_for(vec, keys):
    """theta x (typical score spread of a position over every vector it could see) about 0, 5 and 40; fp32 numbers"""
    v = vec.reshape(-1, vec.shape[-1]).astype(np.float64)
    k = v if keys is None else np.concatenate([v, keys.reshape(-1, keys.shape[-1]).astype(np.float64)])
    d = v.dot(k.T)
    spread = float(np.median(d.max(axis=1) - d.min(axis=1)))
    spread = spread if spread > 0 else max(float(np.abs(d).max()), 1.0)
    return [0.0, float(np.float32(5.0 / spread)), float(np.float32(40.0 / spread))]


def _check(tag, got, vec, val, W, thetas, keys=None, vals=None, group=None):
    p64 = SC.attend_rows(vec, val, W, thetas, keys, vals, group)
    p32 = SC.attend_rows(vec, val, W, thetas, keys, vals, group, np.float32)
    e32, err = _rel_err(p32, p64), _rel_err(got, p64)
    assert err <= max(8 * e32, 1e-6), (tag, err, e32)
    return e32, err


# ------------------------------------------------------------------------------------------------ 1. the causal kernel at its edges
@pytest.mark.parametrize('H', [24, 200, 512])
def test_self_attend_known_answers_at_the_edges(H):
    m = _attend_model(H)
    worst = (0.0, 0.0, '')
    for Mg in SUPPORT:
        rng = np.random.RandomState(100 * H + Mg)
        keys = _vectors(rng, (1, Mg, H)) if Mg else None
        vals = rng.randint(0, N_TOKENS, size=(1, Mg)).astype(np.int32) if Mg else None
        cache = m.cache_from(keys, vals) if Mg else None
        for n_pos in N_POS:
            vec = _vectors(rng, (2, n_pos, H))
            val = rng.randint(0, N_TOKENS, size=(2, n_pos)).astype(np.int32)
            val[1, n_pos // 2] = N_TOKENS                      # a target (and an own value) that occurs nowhere else
            thetas = _thetas_for(vec, keys)
            for W in WINDOWS:
                got = m.cache_self_attend(vec, val, thetas, W, cache=cache)
                assert got.shape == (3, 2, n_pos) and got.dtype == np.float32
                tag = 'H %d Mg %d n_pos %d W %d' % (H, Mg, n_pos, W)
                e32, err = _check(tag, got, vec, val, W, thetas, keys, vals)
                worst = max(worst, (err, e32, tag))
                assert np.all(got[:, 1, n_pos // 2] == 0.0), tag            # entry t holds the target and is never visible
                if Mg == 0:
                    assert np.all(got[:, :, 0] == 0.0), tag                 # the empty set
                    if n_pos > 1:
                        assert np.all(got[:, 0, 1] == (1.0 if val[0, 0] == val[0, 1] else 0.0)), tag    # one entry: all or nothing
            assert _same(got, m.cache_self_attend(vec, val, thetas, WINDOWS[-1], cache=cache))   # two identical calls
        if cache is not None:
            cache.close()
    print('H %d: largest GPU error %.3g (e32 there %.3g) at %s' % ((H,) + worst))


@pytest.mark.parametrize('H', [24, 200, 512])
def test_self_attend_all_scores_negative(H):
    """Even positions live in the first half of the units and odd ones in the second, each with a small negative share of the other
    half, and the support keys are negative everywhere: with W = 1 every score a position sees is negative (theta d <= -5), while the
    masked entries t and t - 2 score large and positive -- scored as anything, they would take nearly all the mass"""
    m = _attend_model(H)
    h2 = H // 2
    for Mg in (0, 17):
        for n_pos in (2, 17, 33, 65):
            rng = np.random.RandomState(7 * n_pos + Mg)
            a = np.abs(rng.normal(size=(1, n_pos, H))) + 0.1
            sign = np.where((np.arange(n_pos) % 2 == 0)[:, None], np.r_[np.ones(h2), -0.1 * np.ones(H - h2)],
                            np.r_[-0.1 * np.ones(h2), np.ones(H - h2)])
            vec = (a * sign[None] / np.sqrt(H)).astype(np.float32)
            val = rng.randint(0, 3, size=(1, n_pos)).astype(np.int32)
            keys = (-(np.abs(rng.normal(size=(1, Mg, H))) + 0.1) / np.sqrt(H)).astype(np.float32) if Mg else None
            vals = rng.randint(0, 3, size=(1, Mg)).astype(np.int32) if Mg else None
            v64 = vec[0].astype(np.float64)
            seen = [v64[t].dot(v64[t - 1]) for t in range(1, n_pos)]
            if Mg:
                seen += list(v64.dot(keys[0].astype(np.float64).T).reshape(-1))
            assert max(seen) < 0 and min(v64[t].dot(v64[t]) for t in range(n_pos)) > 0
            theta = float(np.float32(5.001 / -max(seen)))
            cache = m.cache_from(keys, vals) if Mg else None
            got = m.cache_self_attend(vec, val, [theta, 2 * theta], 1, cache=cache)
            if cache is not None:
                cache.close()
            e32, err = _check('negative H %d Mg %d n_pos %d' % (H, Mg, n_pos), got, vec, val, 1, [theta, 2 * theta], keys, vals)
            print('negative H %d Mg %d n_pos %d: e32 %.3g, GPU %.3g' % (H, Mg, n_pos, e32, err))
            if Mg == 0:                                         # one visible entry: all the mass or none
                assert np.array_equal(got[0, 0, 1:], (val[0, 1:] == val[0, :-1]).astype(np.float32))


@pytest.mark.parametrize('H', [24, 512])
def test_a_masked_key_is_not_scored(H):
    """a key equal to 50 x the query of position t, holding its target, planted at own entry t + 1 and just outside the window; and the
    query's own entry t, which holds the target by definition and scores |q|^2: position t's bits do not move"""
    m = _attend_model(H)
    rng = np.random.RandomState(5)
    n_pos, W, t = 65, 16, 40
    vec = _vectors(rng, (1, n_pos, H))
    val = rng.randint(0, N_TOKENS, size=(1, n_pos)).astype(np.int32)
    keys = _vectors(rng, (1, 17, H))
    vals = rng.randint(0, N_TOKENS, size=(1, 17)).astype(np.int32)
    thetas = _thetas_for(vec, keys)
    cache = m.cache_from(keys, vals)
    for c in (None, cache):
        base = m.cache_self_attend(vec, val, thetas, W, cache=c)
        for where in (t + 1, t - W - 1):
            v2, y2 = vec.copy(), val.copy()
            v2[0, where], y2[0, where] = 50.0 * vec[0, t], val[0, t]
            got = m.cache_self_attend(v2, y2, thetas, W, cache=c)
            assert _same(got[:, 0, t], base[:, 0, t]), where
            assert not _same(got, base)                                     # (the planted key is seen by the positions it belongs to)
        # the row cut off behind position t: entries t + 1 .. are not read at all
        cut = m.cache_self_attend(vec[:, :t + 1], val[:, :t + 1], thetas, W, cache=c)
        assert _same(cut, base[:, :, :t + 1])
        # entry t: give position t a target only entry t holds
        y3 = val.copy()
        y3[0, t] = N_TOKENS
        got = m.cache_self_attend(vec, y3, thetas, W, cache=c)
        assert np.all(got[:, 0, t] == 0.0) and _same(got[:, 0, :t], base[:, 0, :t])
    cache.close()


@pytest.mark.parametrize('H', [24, 200])
def test_self_attend_against_cache_attend_on_the_explicit_list(H):
    m = _attend_model(H)
    rng = np.random.RandomState(11)
    n_pos = 40
    vec = _vectors(rng, (1, n_pos, H))
    val = rng.randint(0, N_TOKENS, size=(1, n_pos)).astype(np.int32)
    keys = _vectors(rng, (1, 17, H))
    vals = rng.randint(0, N_TOKENS, size=(1, 17)).astype(np.int32)
    thetas = _thetas_for(vec, keys)
    cache = m.cache_from(keys, vals)
    for W, c in ((16, None), (1000, None), (17, cache)):
        got = m.cache_self_attend(vec, val, thetas, W, cache=c)
        p64 = SC.attend_rows(vec, val, W, thetas, keys if c else None, vals if c else None)
        p32 = SC.attend_rows(vec, val, W, thetas, keys if c else None, vals if c else None, dtype=np.float32)
        bound = max(8 * _rel_err(p32, p64), 1e-6)
        for t in (1, 15, 16, 17, 33, 39):
            k, v = SC.explicit_entries(vec[0], val[0], t, W, keys[0] if c else None, vals[0] if c else None)
            one = m.cache_from(k[None], v[None].astype(np.int32))
            want = m.cache_attend(one, vec[0, t:t + 1], val[0, t:t + 1], thetas)[:, 0]
            one.close()
            err = _rel_err(got[:, 0, t], want)
            print('H %d W %d t %d: against fsmg_cache_attend %.3g (bound %.3g)' % (H, W, t, err, bound))
            assert err <= bound
    cache.close()


# ------------------------------------------------------------------------------------------------ 2. bitwise
@pytest.mark.parametrize('H', [24, 512])
def test_row_independence_and_permutation(H):
    m = _attend_model(H)
    rng = np.random.RandomState(2)
    n_rows, n_pos, W = 33, 40, 17
    vec = _vectors(rng, (n_rows, n_pos, H))
    val = rng.randint(0, N_TOKENS, size=(n_rows, n_pos)).astype(np.int32)
    keys = _vectors(rng, (2, 17, H))
    vals = rng.randint(0, N_TOKENS, size=(2, 17)).astype(np.int32)
    group = rng.randint(0, 2, size=n_rows).astype(np.int32)
    thetas = _thetas_for(vec[:2], keys)
    cache = m.cache_from(keys, vals)
    for c, g in ((None, None), (cache, group)):
        full = m.cache_self_attend(vec, val, thetas, W, cache=c, group=g)
        assert _same(full, m.cache_self_attend(vec, val, thetas, W, cache=c, group=g))
        for r in (0, 16, 32):
            alone = m.cache_self_attend(vec[r:r + 1], val[r:r + 1], thetas, W, cache=c, group=None if g is None else g[r:r + 1])
            assert _same(alone[:, 0], full[:, r]), r
        perm = rng.permutation(n_rows)
        assert _same(m.cache_self_attend(vec[perm], val[perm], thetas, W, cache=c, group=None if g is None else g[perm]), full[:, perm])
    _check('groups H %d' % H, full, vec, val, W, thetas, keys, vals, group)
    # without a cache the groups are ignored
    assert _same(m.cache_self_attend(vec, val, thetas, W, group=group), m.cache_self_attend(vec, val, thetas, W))
    cache.close()


SCORE_CFGS = {'H24': dict(input_size=60, max_len=40, embedding_size=12, hidden_size=24, n_layers=1),
              'H200x2': dict(input_size=60, max_len=40, embedding_size=12, hidden_size=200, n_layers=2)}


@functools.lru_cache(maxsize=None)
def _score_model(name):
    cfg = small_config(**SCORE_CFGS[name])
    return cfg, new_model(cfg)


def _songs(cfg, rows, seed=0):
    return np.random.RandomState(seed).randint(0, cfg['input_size'], size=(rows, cfg['max_len'])).astype(np.int32)


def _top_hidden(m, cfg, rows):
    d = m.debug_dims()
    T, Hp, H = d['T'], d['Hp'], cfg['hidden_size']
    hs = m.debug_read('h%d' % (cfg['n_layers'] - 1), (T + 1) * rows * Hp).reshape(T + 1, rows, Hp)[1:]
    return np.ascontiguousarray(hs[:, :, :H].transpose(1, 0, 2))


def _ulp_close(got, want32):
    got, want32 = np.asarray(got, np.float32), np.asarray(want32, np.float32)
    fin = np.isfinite(want32)
    return np.array_equal(got[~fin], want32[~fin]) and np.all(np.abs(got[fin].astype(np.float64) - want32[fin]) <= np.spacing(np.abs(want32[fin])))


@pytest.mark.parametrize('name', list(SCORE_CFGS))
def test_score_against_the_gpus_own_vectors(name):
    """max_len 40: two query tiles per row, the second one short, own keys walked with the pass's row stride"""
    cfg, m = _score_model(name)
    T = cfg['max_len']
    support, query = _songs(cfg, 4, seed=1), _songs(cfg, 5, seed=2)
    query[0, T // 2:] = query[0, :T - T // 2]
    group = np.array([0, 1, 1, 0, 1], np.int32)
    thetas, lambdas = [0.0, 2.0, 9.0], [0.0, 0.25, 1.0]
    ALL = dict(logprob=True, cache_prob=True, lstm_logprob=True, row_nll=True)
    cache = m.cache_build(support, n_groups=2)
    for c, g, W in ((None, None, T), (None, None, 7), (cache, group, 17)):
        got = m.cache_self_score(query, thetas, lambdas, W, cache=c, group=g, **ALL)
        assert got['logprob'].shape == (3, 3, 5, T) and got['cache_prob'].shape == (3, 5, T) and got['row_nll'].shape == (3, 3, 5)
        hq = _top_hidden(m, cfg, 5)
        assert _same(got['lstm_logprob'], m.score(query)['logprob'])
        # the pass's hidden states through the raw entry point: the same bits (pad units masked, strided keys)
        assert _same(got['cache_prob'], m.cache_self_attend(hq, query, thetas, W, cache=c, group=g))
        empty = SC.empty_positions(T, c is not None)[None, :]
        for k in range(3):
            for j, lam in enumerate(lambdas):
                assert _ulp_close(got['logprob'][k, j], SC.mix(got['lstm_logprob'], got['cache_prob'][k], lam, empty)), (k, j)
                assert _same(got['row_nll'][k, j], S.row_nll(got['logprob'][k, j]))
                if c is None:                                               # the empty set: the model alone, bitwise, lambda = 1 too
                    assert _same(got['logprob'][k, j][:, 0], got['lstm_logprob'][:, 0])
            assert _same(got['logprob'][k, 0], got['lstm_logprob'])         # lambda = 0
        if c is None:
            assert np.all(got['cache_prob'][:, :, 0] == 0.0)
        assert _same(got['logprob'], m.cache_self_score(query, thetas, lambdas, W, cache=c, group=g)['logprob'])     # twice
        win = m.cache_self_score(query, thetas, lambdas, W, cache=c, group=g, nll_first=4, nll_count=5, **ALL)
        assert _same(win['row_nll'][1, 1], S.row_nll(got['logprob'][1, 1], 4, 5))
        for key in ALL:
            only = m.cache_self_score(query, thetas, lambdas, W, cache=c, group=g, nll_first=4, nll_count=5, **{k: k == key for k in ALL})
            assert set(only) == {key} and _same(only[key], win[key]), key
        # passes: rows 3 at a time are the bits of the pieces scored in calls of their own
        p3 = m.cache_self_score(query, thetas, lambdas, W, cache=c, group=g, pass_rows=3, **ALL)
        a = m.cache_self_score(query[:3], thetas, lambdas, W, cache=c, group=None if g is None else g[:3], **ALL)
        b = m.cache_self_score(query[3:], thetas, lambdas, W, cache=c, group=None if g is None else g[3:], **ALL)
        for key, axis in (('logprob', 2), ('cache_prob', 1), ('lstm_logprob', 0), ('row_nll', 2)):
            assert _same(p3[key], np.concatenate([a[key], b[key]], axis=axis)), key
    # the copied half at a sharp theta and W = T: the mixture beats the model on that row
    got = m.cache_self_score(query[:1], [9.0], [0.25], T, lstm_logprob=True)
    print('%s: copied-half row %.4f mixed against %.4f LSTM (GPU parameters, untrained)'
          % (name, float(got['row_nll'][0, 0, 0]), float(-got['lstm_logprob'][0].astype(np.float64).mean())))
    cache.close()


def test_the_support_set_entry_points_keep_their_bits():
    cfg, m = _score_model('H24')
    T = cfg['max_len']
    support, query = _songs(cfg, 4, seed=1), _songs(cfg, 5, seed=2)
    group = np.array([0, 1, 1, 0, 1], np.int32)
    thetas, lambdas = [0.0, 2.0, 9.0], [0.0, 0.25, 1.0]
    fresh = new_model(cfg)                              # a handle on which no self entry point has run
    cache0 = fresh.cache_build(support, n_groups=2)
    q = _vectors(np.random.RandomState(3), (9, cfg['hidden_size']))
    y = np.arange(9, dtype=np.int32) % 5

    def snapshot(model, cache):
        sc = model.cache_score(cache, query, thetas, lambdas, group=group, cache_prob=True, lstm_logprob=True)
        at = model.cache_attend(cache, q, y, thetas, group=(np.arange(9) % 2).astype(np.int32))
        keys, vals = cache.get()
        toks, lps = model.cache_generate(cache, 5, 6, 2.0, 0.25, group=group, seed=4, primer=query[:, :3], logprobs=True)
        return [sc['logprob'], sc['cache_prob'], sc['lstm_logprob'], sc['row_nll'], at, keys, vals, toks, lps]

    before = snapshot(fresh, cache0)
    fresh.cache_self_score(query, thetas, lambdas, 7, cache=cache0, group=group)
    fresh.cache_self_score(query, thetas, lambdas, T)
    fresh.cache_self_attend(_vectors(np.random.RandomState(4), (2, 33, cfg['hidden_size'])), np.zeros((2, 33), np.int32), thetas, 5, cache=cache0)
    after = snapshot(fresh, cache0)
    for i, (a, b) in enumerate(zip(before, after)):
        assert _same(a, b), i
    cache0.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------ 3. score against the fp64 oracle
def _visible_l1(hq_r, keys_g, T, W):
    """per position: sum_j |q_j| + the largest sum_j |k_ij| over the entries the position sees (0 where it sees none)"""
    own = np.abs(hq_r).sum(axis=1)
    sup = float(np.abs(keys_g).sum(axis=1).max()) if keys_g is not None else 0.0
    out = np.empty(T)
    for t in range(T):
        lo = max(0, t - W)
        kmax = max(sup, float(own[lo:t].max()) if t > lo else 0.0)
        out[t] = own[t] + kmax if kmax > 0 else 0.0
    return out


@pytest.mark.parametrize('name', ['H24', 'H200x2', 'H512'])
def test_score_against_the_fp64_oracle(name):
    case = SC.oracle_case(name)
    cfg, params, query, group, thetas = case['cfg'], case['params'], case['query'], case['group'], case['thetas']
    T = cfg['max_len']
    m = new_model(cfg, params=params)
    cache = m.cache_build(case['support'], n_groups=2)
    for with_support, W in ((False, T), (False, 5), (True, 5)):
        want = SC.score(params, query, W, thetas, SC.LAMBDAS, cfg, support=case['support'] if with_support else None, n_groups=2,
                        group=group if with_support else None)
        got = m.cache_self_score(query, thetas, SC.LAMBDAS, W, cache=cache if with_support else None, group=group, lstm_logprob=True)
        e_lstm = float(np.abs(got['lstm_logprob'] - want['lstm_logprob']).max())
        assert e_lstm <= 1e-4
        l1 = np.stack([_visible_l1(want['queries'][r], want['keys'][group[r]] if with_support else None, T, W) for r in range(5)])
        for k, th in enumerate(thetas):
            bound = 1e-4 + th * 2e-5 * l1
            for j, lam in enumerate(SC.LAMBDAS):
                w, g = want['logprob'][k, j], got['logprob'][k, j].astype(np.float64)
                fin = np.isfinite(w)
                assert np.array_equal(g[~fin], w[~fin])                     # lambda = 1 where no visible entry holds the target: -inf
                err = np.abs(g[fin] - w[fin])
                print('%s support %d W %d theta %.3g lambda %.2f: log-prob error %.3g (bound %.3g .. %.3g), LSTM %.3g'
                      % (name, with_support, W, th, lam, err.max(), bound.min(), bound.max(), e_lstm))
                assert np.all(err <= bound[fin]), (with_support, W, k, j)
    cache.close()
    # the copied-half song: the GPU's per-token gain against the fp64 gain test_selfcache_cpu records
    theta, gain64, kept = SC.gain_theta(case)
    got = m.cache_self_score(query[:1], [theta], [SC.GAIN_LAMBDA], T, lstm_logprob=True)
    gain = SC.copied_half_gain(got['logprob'][0, 0, 0], got['lstm_logprob'][0])
    hq = R.oracle_hidden(params, query[:1], cfg)[0][0]
    bound = float((1e-4 + theta * 2e-5 * _visible_l1(hq, None, T, T)).max())
    print('%s: copied-half gain %.5f on the GPU, %.5f in fp64 (theta %.3g, %s; bound %.3g)'
          % (name, gain, gain64, theta, 'the default' if kept else "tune's grid", bound))
    assert gain64 > 0 and abs(gain - gain64) <= bound
    m.close()


# ------------------------------------------------------------------------------------------------ 4. the plugin
class _Episode(object):
    def __init__(self, support, query):
        self.support, self.query = support, query


def test_plugin_uses_the_union_when_cache_self_is_set(tmp_path):
    from models.cache_lstm import CacheLSTM
    base_cfg = dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name='cache_lstm',
                    cache_theta=1.5, cache_lambda=0.25)
    plain = CacheLSTM(dict(base_cfg, checkpt_dir=str(tmp_path / 'plain')))
    both = CacheLSTM(dict(base_cfg, checkpt_dir=str(tmp_path / 'both'), cache_self=True, cache_window=5))
    plain.recover_or_init('')
    both.recover_or_init('')
    both.engine.set_params(plain.engine.get_params())
    rng = np.random.RandomState(5)
    episodes = []
    for _ in range(2):
        support = rng.randint(0, 40, size=(3, 2, 12)).astype(np.int32)
        query = rng.randint(0, 40, size=(3, 4, 12)).astype(np.int32)
        query[:, 0, 6:] = query[:, 0, :6]
        episodes.append(_Episode(support, query))
    ep = episodes[0]
    m = both.engine
    group = np.repeat(np.arange(3), 4).astype(np.int32)
    cache = m.cache_build(ep.support, n_groups=3)
    lp = m.cache_self_score(ep.query, [1.5], [0.25], 5, cache=cache, group=group)['logprob']
    want = float(-lp.astype(np.float64).mean())
    assert both.eval(ep) == want and both.eval_many(episodes) == [both.eval(e) for e in episodes]
    thetas, lambdas = [0.0, 1.5, 4.0], [0.0, 0.25, 1.0]
    grid = both.tune(episodes, thetas, lambdas)
    assert grid.shape == (3, 3) and abs(grid[1, 1] - np.mean([both.eval(e) for e in episodes])) <= 1e-12
    # cache_self unset: the paths are what they were
    assert plain.eval(ep) == plain.engine.cache_eval_step(ep.support, ep.query, 1.5, 0.25)
    assert abs(plain.tune(episodes, thetas, lambdas)[1, 1] - np.mean([plain.eval(e) for e in episodes])) <= 1e-6
    assert abs(grid[0, 0] - plain.tune(episodes, thetas, lambdas)[0, 0]) <= 1e-6               # lambda = 0: the model alone
    songs = ep.query.reshape(-1, 12)
    one = m.cache_build(ep.support.reshape(-1, 12), n_groups=1)
    assert _same(both.score(ep.support, songs)['logprob'], m.cache_self_score(songs, [1.5], [0.25], 5, cache=one)['logprob'])
    assert _same(plain.score(ep.support, songs)['logprob'], m.cache_score(one, songs, [1.5], [0.25])['logprob'])
    for model in (plain, both):                         # no support set at all
        assert _same(model.score_self(songs, window=5)['logprob'], m.cache_self_score(songs, [1.5], [0.25], 5)['logprob'])
    one.close()
    cache.close()


# ------------------------------------------------------------------------------------------------ 5. errors
def test_argument_errors():
    from fsmg import binding as B
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m, m2 = new_model(cfg), new_model(cfg)
    lib = m._lib
    songs = np.random.RandomState(0).randint(0, 50, size=(4, 8)).astype(np.int32)
    F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    cache = m.cache_build(songs, n_groups=2)
    SENTINEL = np.float32(-123.5)
    lp = np.full((1, 1, 4, 8), SENTINEL, np.float32)
    pr = np.full((1, 2, 5), SENTINEL, np.float32)
    vec = np.zeros((2, 5, 16), np.float32)
    val = np.zeros((2, 5), np.int32)

    def selfcfg(**over):
        sc = m.cache_self_config(3)
        for k, v in over.items():
            if k == 'reserved':
                sc.reserved[v] = 1
            else:
                setattr(sc, k, v)
        return sc

    def score(handle=None, c_ptr=None, tokens=songs, group=None, out=lp, theta0=None, lambda0=None, self_null=False, cfg_over=None, **over):
        c = m.cache_score_config(4, [1.0], [0.5])
        for k, v in (cfg_over or {}).items():
            setattr(c, k, v)
        if theta0 is not None:
            c.thetas[0] = theta0
        if lambda0 is not None:
            c.lambdas[0] = lambda0
        sc = selfcfg(**over)
        lp[...] = SENTINEL
        g = None if group is None else np.asarray(group, np.int32)
        rc = lib.fsmg_cache_self_score((handle or m)._h, c_ptr, C.byref(c), None if self_null else C.byref(sc),
                                       None if tokens is None else C.c_void_p(tokens.ctypes.data),
                                       None if g is None else g.ctypes.data_as(I32P), None if out is None else out.ctypes.data_as(F32P),
                                       None, None, None)
        if rc != 0:
            assert lib.fsmg_last_error((handle or m)._h) and np.all(lp == SENTINEL), 'a refused call leaves a message and the outputs alone'
        return rc

    def attend(c_ptr=None, n_rows=2, n_pos=5, values=val, group=None, thetas=(1.0,), n_theta=1, self_null=False, **over):
        sc = selfcfg(**over)
        th = np.asarray(thetas, np.float32)
        pr[...] = SENTINEL
        g = None if group is None else np.asarray(group, np.int32)
        rc = lib.fsmg_cache_self_attend(m._h, c_ptr, None if self_null else C.byref(sc), n_rows, n_pos, vec.ctypes.data_as(F32P),
                                        values.ctypes.data_as(I32P), None if g is None else g.ctypes.data_as(I32P),
                                        th.ctypes.data_as(F32P), n_theta, pr.ctypes.data_as(F32P))
        if rc != 0:
            assert lib.fsmg_last_error(m._h) and np.all(pr == SENTINEL), 'a refused call leaves a message and the outputs alone'
        return rc

    assert score(version=2) == -1 and score(version=0) == -1 and attend(version=2) == -1            # wrong version
    assert score(reserved=0) == -1 and score(reserved=13) == -1 and attend(reserved=5) == -1        # nonzero reserved
    assert score(window=0) == -1 and score(window=-3) == -1 and attend(window=0) == -1              # window < 1
    assert score(self_null=True) == -1 and attend(self_null=True) == -1
    # what fsmg_cache_score refuses
    assert score(cfg_over=dict(version=0)) == -1 and score(cfg_over=dict(n_theta=9)) == -1 and score(cfg_over=dict(n_lambda=0)) == -1
    assert score(theta0=-0.5) == -1 and score(theta0=float('nan')) == -1 and score(lambda0=1.01) == -1
    assert score(out=None) == -1 and score(tokens=None) == -1 and score(cfg_over=dict(nll_first=8)) == -1
    assert score(c_ptr=cache._c, group=[0, 2, 0, 0]) == -1                   # group id out of range
    assert score(handle=m2, c_ptr=cache._c) == -1                            # another handle's cache
    bad = songs.copy()
    bad[2, 3] = 50
    assert score(tokens=bad) == -7                                           # token out of range
    # what fsmg_cache_attend refuses
    assert attend(n_rows=0) == -1 and attend(n_pos=0) == -1 and attend(n_rows=1 << 12, n_pos=(1 << 10) + 1) == -1
    assert attend(n_theta=0) == -1 and attend(n_theta=9) == -1 and attend(thetas=(-1.0,)) == -1 and attend(thetas=(float('inf'),)) == -1
    assert attend(c_ptr=cache._c, group=[0, 2]) == -1
    badv = val.copy()
    badv[1, 4] = 51
    assert attend(values=badv) == -7                                         # value outside [0, input_size]
    badv[1, 4] = -1
    assert attend(values=badv) == -7
    okv = val.copy()
    okv[1, 4] = 50                                                           # input_size itself is a legal value
    assert attend(values=okv) == 0 and not np.any(pr == SENTINEL)
    # group is ignored without a cache; the good calls work, with and without one
    assert score(group=[0, 9, -1, 0]) == 0 and not np.any(lp == SENTINEL)
    assert score(c_ptr=cache._c, group=[0, 1, 1, 0]) == 0 and attend(c_ptr=cache._c, group=[1, 0]) == 0
    with pytest.raises(ValueError):
        m.cache_self_attend(np.zeros((2, 5, 15), np.float32), val, [1.0], 3)
    with pytest.raises(ValueError):
        m.cache_self_score(songs, [1.0], [0.5], 3, group=[0, 1])
    # a destroyed cache: an error, not a crash; the handle stays usable
    handle = cache._c
    cache.close()
    assert score(c_ptr=handle) == -1 and attend(c_ptr=handle) == -1
    assert np.all(np.isfinite(m.cache_self_score(songs, [1.0], [0.5], 3)['logprob']))
    m.close()
    m2.close()
