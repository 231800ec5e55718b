"""Cache-conditioned generation (include/fsmg.h fsmg_cache_generate / fsmg_dstate_cache_generate / fsmg_cache_distribution) on the
MI355X: the whole mixed distribution against fp64 at tile and chunk edges, its agreement with fsmg_cache_attend, the bitwise
promises (row independence, group isolation, lambda = 0, determinism, the state composition laws, no side effects), the decoder
against the GPU's own vectors and, teacher-forced, against the fp64 oracle, the plugin and the argument errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import cache_ref as CR
import cachegen_ref as R
import gen_ref as G
from conftest import small_config
from gpu_utils import new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

START = 97                      # the start word of the distribution tests' models (input_size 97, V1 = 98)
PALETTE = np.array([0, 3, 5, 11, 42, 96, START], np.int32)     # few values: every held column has several entries; 50 occurs nowhere
LAMBDAS = (0.0, 0.25, 1.0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, want64):
    """max relative error over want > 0; where want == 0 the result must be exactly 0"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    pos = want64 > 0
    assert np.all(got[~pos] == 0.0), 'a column no entry holds must give exactly 0'
    return float((np.abs(got[pos] - want64[pos]) / want64[pos]).max()) if pos.any() else 0.0


def _ulp_close(got, want32):
    got, want32 = np.asarray(got, np.float32), np.asarray(want32, np.float32)
    fin = np.isfinite(want32)
    return np.array_equal(got[~fin], want32[~fin]) and np.all(np.abs(got[fin].astype(np.float64) - want32[fin]) <= np.spacing(np.abs(want32[fin])))


@functools.lru_cache(maxsize=None)
def _dist_model(H, input_size=START):
    return new_model(small_config(input_size=input_size, max_len=4, embedding_size=8, hidden_size=H))


def _own_scores(keys, q, group):
    k64, q64 = keys.astype(np.float64), q.astype(np.float64)
    return [q64[i].dot(k64[group[i]].T) for i in range(q.shape[0])]


def _thetas_for(keys, q, group):
    """theta (d_max - d_min) about 0, about 5 and about 40 for the typical query; fp32 numbers, so that the library (whose theta is a
    float) and both modes of the restatement see the same inputs"""
    d = _own_scores(keys, q, group)
    spread = float(np.median([x.max() - x.min() for x in d]))
    spread = spread if spread > 0 else float(max(np.abs(x).max() for x in d))
    return [0.0, float(np.float32(5.0 / spread)), float(np.float32(40.0 / spread))]


def _check_distribution(tag, m, cache, keys, vals, q, z, group, theta, lambdas=LAMBDAS):
    """one (inputs, theta) against the restatement for every lambda; -> (e32, GPU error) of p_cache"""
    ref = R.distribution(keys, vals, q, z, group, theta, 0.0)
    p32 = R.distribution(keys, vals, q, z, group, theta, 0.0, np.float32)['cache_prob']
    e32 = _rel_err(p32, ref['cache_prob'])
    err = None
    for lam in lambdas:
        got = m.cache_distribution(cache, q, z, theta, lam, group=group)
        pc, zz, lse = got['cache_prob'], got['logprob'], got['lse']
        assert pc.shape == z.shape and zz.shape == z.shape and lse.shape == (z.shape[0],)
        if err is None:
            err, first = _rel_err(pc, ref['cache_prob']), pc
            assert err <= max(8 * e32, 1e-6), (tag, err, e32)
            assert np.all(np.abs(pc.astype(np.float64).sum(axis=1) - 1.0) <= 1e-6), tag
            assert np.all(np.abs(lse - ref['lse']) <= 1e-5), tag
        assert _same(pc, first), (tag, lam)                                 # p_cache does not depend on lambda
        lp = z - lse[:, None]                                               # fl32(z - lse): an fp32 subtraction
        assert lp.dtype == np.float32
        assert _ulp_close(zz, CR.mix(lp, pc, lam)), (tag, lam)
        if lam == 0.0:
            assert _same(zz, lp), tag                                       # lambda = 0: lp bitwise
        if lam == 1.0:
            assert np.all(zz[pc == 0] == -np.inf), tag
    return e32, err


def _inputs(rng, Mg, H, n, V1=START + 1, palette=PALETTE, scale=3.0):
    keys = (rng.normal(size=(2, Mg, H)) / np.sqrt(H)).astype(np.float32)
    vals = palette[rng.randint(0, len(palette), size=(2, Mg))].astype(np.int32)
    vals[0, 0] = palette[-1]                                                # the start word is held
    q = (rng.normal(size=(n, H)) * scale).astype(np.float32)
    z = (rng.normal(size=(n, V1)) * 2).astype(np.float32)
    group = (np.arange(n) % 2).astype(np.int32) if n > 1 else np.zeros(1, np.int32)
    return keys, vals, q, z, group


# ------------------------------------------------------------------------------------------------ 1. the distribution at tile and chunk edges
@pytest.mark.parametrize('H', [24, 200, 512])
def test_distribution_at_tile_and_chunk_edges(H):
    from fsmg.binding import FSMG_CACHE_GEN_CHUNK as CHUNK
    m = _dist_model(H)
    worst = (0.0, 0.0)
    # 1 .. 257: the 16-key tile and its tails; 3 * CHUNK + 5: four key chunks, the last one ragged
    for Mg in (1, 15, 16, 17, 65, 257, 3 * CHUNK + 5):
        for n in (1, 17, 33):
            rng = np.random.RandomState(1000 * Mg + n)
            keys, vals, q, z, group = _inputs(rng, Mg, H, n)
            cache = m.cache_from(keys, vals)
            for theta in _thetas_for(keys, q, group):
                tag = 'H %d Mg %d n %d theta %.4g' % (H, Mg, n, theta)
                e32, err = _check_distribution(tag, m, cache, keys, vals, q, z, group, theta)
                print('%s: e32 %.3g, GPU %.3g' % (tag, e32, err))
                worst = max(worst, (e32, err), key=lambda p: p[1])
            if Mg == 1:                                                      # one entry: all the mass
                pc = m.cache_distribution(cache, q, z, 1.0, 0.25, group=group)['cache_prob']
                assert np.all(pc[np.arange(n), vals[group, 0]] == 1.0) and np.all(pc.sum(axis=1) == 1.0)
            cache.close()
    print('H %d: largest GPU error %.3g (e32 there %.3g)' % (H, worst[1], worst[0]))


@pytest.mark.parametrize('H', [24, 200, 512])
def test_distribution_all_scores_negative_masks_the_tail(H):
    """keys = -|.| against queries = +|.| with theta d <= -5: a pad key scored as zero would take nearly all the mass"""
    from fsmg.binding import FSMG_CACHE_GEN_CHUNK as CHUNK
    m = _dist_model(H)
    for Mg in (1, 15, 17, 3 * CHUNK + 5, 65):
        rng = np.random.RandomState(Mg)
        keys, vals, q, z, group = _inputs(rng, Mg, H, 17)
        keys, q = -np.abs(keys), np.abs(q) / 3
        dmax = max(x.max() for x in _own_scores(keys, q, group))
        assert dmax < 0
        theta = float(np.float32(5.001 / -dmax))
        cache = m.cache_from(keys, vals)
        for th in (theta, 2 * theta):
            e32, err = _check_distribution('negative H %d Mg %d' % (H, Mg), m, cache, keys, vals, q, z, group, th, lambdas=(0.25,))
            print('negative H %d Mg %d theta %.4g: e32 %.3g, GPU %.3g' % (H, Mg, th, e32, err))
        cache.close()


def test_distribution_over_a_large_vocabulary():
    V = 40000
    m = _dist_model(24, V)
    rng = np.random.RandomState(8)
    palette = np.array([0, 1, 255, 256, 1023, 1024, 20000, 39999, V], np.int32)
    keys, vals, q, z, group = _inputs(rng, 65, 24, 3, V1=V + 1, palette=palette)
    cache = m.cache_from(keys, vals)
    for theta in _thetas_for(keys, q, group)[1:]:
        e32, err = _check_distribution('V1 40001 theta %.4g' % theta, m, cache, keys, vals, q, z, group, theta)
        print('V1 40001 theta %.4g: e32 %.3g, GPU %.3g' % (theta, e32, err))
    cache.close()


# ------------------------------------------------------------------------------------------------ 2. agreement with fsmg_cache_attend
@pytest.mark.parametrize('H', [24, 512])
def test_distribution_agrees_with_cache_attend(H):
    m = _dist_model(H)
    rng = np.random.RandomState(5)
    keys, vals, q, z, group = _inputs(rng, 65, H, 33)
    y = PALETTE[rng.randint(0, len(PALETTE), size=33)].astype(np.int32)
    y[1] = 50                                                               # a target no entry holds
    thetas = _thetas_for(keys, q, group)
    cache = m.cache_from(keys, vals)
    att = m.cache_attend(cache, q, y, thetas, group=group)
    p64 = CR.attend_groups(keys, vals, q, y, group, thetas)
    p32 = CR.attend_groups(keys, vals, q, y, group, thetas, np.float32)
    for k, theta in enumerate(thetas):
        pc = m.cache_distribution(cache, q, z, theta, 0.25, group=group)['cache_prob'][np.arange(33), y]
        e32 = _rel_err(p32[k], p64[k])
        pos = p64[k] > 0
        assert np.all(pc[~pos] == 0) and np.all(att[k][~pos] == 0)
        diff = float((np.abs(pc[pos].astype(np.float64) - att[k][pos]) / p64[k][pos]).max())
        print('H %d theta %.4g: distribution against attend %.3g (e32 %.3g)' % (H, theta, diff, e32))
        assert diff <= max(8 * e32, 1e-6)
    cache.close()


# ------------------------------------------------------------------------------------------------ 3. row independence, group isolation, repeatability
@pytest.mark.parametrize('H', [24, 512])
def test_distribution_rows_are_their_own(H):
    m = _dist_model(H)
    rng = np.random.RandomState(3)
    Mg, n = 65, 33
    keys, vals, q, z, _ = _inputs(rng, Mg, H, n)
    group = rng.randint(0, 2, size=n).astype(np.int32)
    theta = _thetas_for(keys, q, group)[1]
    KEYS = ('cache_prob', 'logprob', 'lse')
    two = m.cache_from(keys, vals)
    bytes0 = two.info()['bytes']
    base = m.cache_distribution(two, q, z, theta, 0.25, group=group)
    assert two.info()['bytes'] > bytes0                                     # the value index, built on first use ...
    bytes1 = two.info()['bytes']
    again = m.cache_distribution(two, q, z, theta, 0.25, group=group)
    assert two.info()['bytes'] == bytes1                                    # ... once
    for key in KEYS:
        assert _same(base[key], again[key]), key                            # two identical calls: identical bits
    for i in (0, 16, 32):                                                   # a row alone gives the bits it gives among 33
        alone = m.cache_distribution(two, q[i:i + 1], z[i:i + 1], theta, 0.25, group=group[i:i + 1])
        for key in KEYS:
            assert _same(alone[key], base[key][i:i + 1]), (key, i)
    perm = rng.permutation(n)
    shuffled = m.cache_distribution(two, q[perm], z[perm], theta, 0.25, group=group[perm])
    for key in KEYS:
        assert _same(shuffled[key], base[key][perm]), key
    # the rows of group 0 against a one-group cache, and with every row of the call in group 0 (group NULL)
    one = m.cache_from(keys[:1], vals[:1])
    g0 = np.flatnonzero(group == 0)
    single = m.cache_distribution(one, q[g0], z[g0], theta, 0.25)
    for key in KEYS:
        assert _same(single[key], base[key][g0]), key
    # in the OTHER group: a key equal to 50 x the query, holding a value absent from the row's own group -- it must not be seen
    assert not np.any(vals == 50)
    planted_k, planted_v = keys.copy(), vals.copy()
    for j, i in enumerate(g0[:Mg]):
        planted_k[1, j], planted_v[1, j] = 50.0 * q[i], 50
    planted = m.cache_from(planted_k, planted_v)
    seen = m.cache_distribution(planted, q, z, theta, 0.25, group=group)
    for key in KEYS:
        assert _same(seen[key][g0], base[key][g0]), key
    assert np.all(seen['cache_prob'][g0, 50] == 0)
    there = m.cache_distribution(planted, q[g0], z[g0], theta, 0.25, group=np.ones(len(g0), np.int32))
    assert np.all(there['cache_prob'][:, 50] > 0.99)                        # in its own group the planted key IS seen
    # the outputs that were there before keep their bits once the index exists
    y = vals[group, 0]
    fresh = m.cache_from(keys, vals)
    assert _same(m.cache_attend(fresh, q, y, [theta], group=group), m.cache_attend(two, q, y, [theta], group=group))
    assert _same(fresh.get()[0], two.get()[0]) and np.array_equal(fresh.get()[1], two.get()[1])
    for c in (one, two, planted, fresh):
        c.close()


# ------------------------------------------------------------------------------------------------ shared: a trained model and a two-group cache
def _trained(cfg, steps=3, seed=7):
    m = new_model(cfg)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


GEN_CFG = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
GEN_GROUP = np.array([0, 0, 1, 1, 0], np.int32)


@functools.lru_cache(maxsize=None)
def _gen_setup():
    """a model after three train steps; a cache built from 4 songs in 2 groups whose tokens are disjoint: group 0 holds ids below 40,
    group 1 ids in [50, 90)"""
    m = _trained(GEN_CFG)
    rng = np.random.RandomState(2)
    songs = np.concatenate([rng.randint(0, 40, size=(2, 12)), rng.randint(50, 90, size=(2, 12))]).astype(np.int32)
    cache = m.cache_build(songs, n_groups=2)
    primer = np.stack([songs[2 * g, :3] for g in GEN_GROUP]).astype(np.int32)
    keys = cache.get()[0].astype(np.float64)
    dmax = max(float(np.abs(keys[g].dot(keys[g].T)).max()) for g in range(2))
    return m, cache, songs, primer, float(np.float32(5.0 / dmax))


def _state(m):
    opt = {k: m.get_opt_state(k) for k in m.param_shapes}
    return m.get_params(), opt, m.step, m.read_losses(2), m.stats()


def _same_state(a, b):
    pa, oa, sa, la, ta = a
    pb, ob, sb, lb, tb = b
    for k in pa:
        assert np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)), k
        assert np.array_equal(oa[k][0], ob[k][0]) and np.array_equal(oa[k][1], ob[k][1]), k
    assert sa == sb and np.array_equal(la, lb) and ta == tb


def _same_dstate(a, b):
    ga, gb = a.get(), b.get()
    return all(_same(ga[k], gb[k]) for k in ('h', 'c', 'ctx')) and (ga['n_ctx'], ga['n_gen']) == (gb['n_ctx'], gb['n_gen'])


FILTERS = dict(top_p=0.9, min_p=0.01, repetition_penalty=1.3, repeat_window=4)


# ------------------------------------------------------------------------------------------------ 4. generate: the exact properties
def test_generate_lambda_zero_is_generate_bitwise():
    m, cache, songs, primer, theta = _gen_setup()
    for kw in (dict(), FILTERS):
        kw = dict(kw, temperature=0.9, top_k=7, seed=11, logprobs=True)
        want = m.generate(5, 9, primer=primer, **kw)
        got = m.cache_generate(cache, 5, 9, theta, 0.0, group=GEN_GROUP, primer=primer, **kw)
        assert np.array_equal(got[0], want[0]) and _same(got[1], want[1])
        a, b = m.new_state(5, history=64), m.new_state(5, history=64)
        m.feed(a, primer)
        m.feed(b, primer)
        want = m.generate(5, 9, state=a, **kw)
        got = m.cache_generate(cache, 5, 9, theta, 0.0, group=GEN_GROUP, state=b, **kw)
        assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and _same_dstate(a, b)
        a.close()
        b.close()


def test_generate_draws_from_the_rows_own_group_deterministically():
    m, cache, songs, primer, theta = _gen_setup()
    before = _state(m)
    kw = dict(temperature=1.0, seed=4, logprobs=True, primer=primer)
    # lambda = 1: every token is a value of the row's group, never one of the other group's
    toks, lps = m.cache_generate(cache, 5, 12, theta, 1.0, group=GEN_GROUP, **kw)
    held = [set(songs[:2].reshape(-1)), set(songs[2:].reshape(-1))]
    for b in range(5):
        assert set(toks[b]) <= held[GEN_GROUP[b]], b
    assert np.all(np.isfinite(lps)) and np.all(lps <= 1e-6)
    # the mixture: identical calls, identical bits; a row does not depend on n_seq, on the other rows or on their groups
    for extra in (dict(), FILTERS, dict(top_k=5, temperature=0.7)):
        k2 = dict(kw, **extra)
        base = m.cache_generate(cache, 5, 12, theta, 0.25, group=GEN_GROUP, **k2)
        again = m.cache_generate(cache, 5, 12, theta, 0.25, group=GEN_GROUP, **k2)
        assert np.array_equal(base[0], again[0]) and _same(base[1], again[1])
        fewer = m.cache_generate(cache, 3, 12, theta, 0.25, group=GEN_GROUP[:3], **dict(k2, primer=primer[:3]))
        assert np.array_equal(fewer[0], base[0][:3]) and _same(fewer[1], base[1][:3])
        other = np.array([0, 1, 1, 0, 0], np.int32)                         # rows 1 and 3 change their group
        mixed = m.cache_generate(cache, 5, 12, theta, 0.25, group=other, **k2)
        for b in (0, 2, 4):
            assert np.array_equal(mixed[0][b], base[0][b]) and _same(mixed[1][b], base[1][b]), b
    assert not np.array_equal(base[0], m.generate(5, 12, **k2)[0])           # the cache is felt
    # group NULL = all 0
    zero = m.cache_generate(cache, 5, 12, theta, 0.25, group=np.zeros(5, np.int32), **kw)
    none = m.cache_generate(cache, 5, 12, theta, 0.25, **kw)
    assert np.array_equal(zero[0], none[0]) and _same(zero[1], none[1])
    z = np.zeros((2, 98), np.float32)
    m.cache_distribution(cache, np.ones((2, 32), np.float32), z, theta, 0.25)
    _same_state(before, _state(m))                                          # no handle state is changed


def test_generate_state_composition_laws():
    m, cache, songs, primer, theta = _gen_setup()
    for extra in (dict(), FILTERS):
        kw = dict(extra, temperature=0.8, top_k=6, seed=17, logprobs=True)
        one_shot = m.cache_generate(cache, 5, 11, theta, 0.25, group=GEN_GROUP, primer=primer, **kw)
        a, b = m.new_state(5, history=64), m.new_state(5, history=64)
        m.feed(a, primer)
        m.feed(b, primer)
        whole = m.cache_generate(cache, 5, 11, theta, 0.25, group=GEN_GROUP, state=a, **kw)
        parts = [m.cache_generate(cache, 5, n, theta, 0.25, group=GEN_GROUP, state=b, **kw) for n in (4, 1, 6)]
        toks, lps = np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 1)
        assert np.array_equal(whole[0], toks) and _same(whole[1], lps) and _same_dstate(a, b)       # generate(a) then (b) = (a + b)
        assert np.array_equal(whole[0], one_shot[0]) and _same(whole[1], one_shot[1])               # fresh, feed(primer), generate
        assert a.info()['n_gen'] == 11 and a.info()['n_ctx'] == 3 + 11
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 5. generate against the GPU's own vectors
def test_generate_against_the_gpus_own_vectors():
    """One generated position from a state: the query is the state's top-layer h, the logits row is fsmg_score's at the same prefix,
    and fsmg_cache_distribution gives z''.  The decode cells and the scoring pass are different kernels: where their hidden states
    agree in bits the token must be the Gumbel-max of z'' at Philox position n_gen and the log-prob z''_tok - lse(z'') to 1 ulp;
    where they do not, the difference is printed and the margin form holds: the token's perturbed score is within the mixed row's
    tolerance (cachegen_ref.tolerance) of the maximum, its log-prob within it, and the token is the maximum's wherever the margin is
    twice that."""
    m, cache, songs, primer, theta = _gen_setup()
    V1, L, T = 98, GEN_CFG['n_layers'], GEN_CFG['max_len']
    keys = cache.get()[0].astype(np.float64)
    for temperature, top_k, seed in ((1.0, 0, 31), (0.7, 5, 32)):
        st = m.new_state(5, history=64)
        m.feed(st, primer)
        toks, lps = m.cache_generate(cache, 5, 1, theta, 0.25, group=GEN_GROUP, state=st, temperature=temperature, top_k=top_k, seed=seed,
                                     logprobs=True)
        h = st.get()['h'][L - 1]                                             # the queries of that position
        st.close()
        rows = np.zeros((5, T), np.int32)
        rows[:, :3] = primer                                                 # position 3 of a scored row: after [start, primer]
        m.score(rows)
        d = m.debug_dims()
        z = m.debug_read('logits', T * 5 * d['V1p']).reshape(T, 5, d['V1p'])[3, :, :V1].copy()
        hs = m.debug_read('h%d' % (L - 1), (T + 1) * 5 * d['Hp']).reshape(T + 1, 5, d['Hp'])[4, :, :GEN_CFG['hidden_size']]
        exact = _same(hs, h)
        print('T %.1f top_k %d: hidden states of the decode cells and of the scoring pass %s (largest difference %.3g)'
              % (temperature, top_k, 'agree in bits' if exact else 'differ', float(np.abs(hs.astype(np.float64) - h).max())))
        zz = m.cache_distribution(cache, h, z, theta, 0.25, group=GEN_GROUP)['logprob'].astype(np.float64)
        for b in range(5):
            g = int(toks[b, 0])
            noise = G.gumbel(seed, 0, b, V1)                                 # Philox position n_gen + t = 0
            want, score = G.choose(zz[b], temperature, top_k, noise)
            want_lp = zz[b, g] - G.logsumexp(zz[b])
            margin = R._margin(score)
            if exact:
                assert g == want or margin < 1e-5, (b, g, want, margin)
                assert _ulp_close(lps[b, 0], np.float32(want_lp)), (b, lps[b, 0], want_lp)
                continue
            tol = R.tolerance(theta, R.l1_of(h[b].astype(np.float64), keys[GEN_GROUP[b]]))
            sg = zz[b, g] / temperature + noise[g]
            print('  row %d: log-prob error %.3g, perturbed score %.3g below the maximum, margin %.3g (tolerance %.3g)'
                  % (b, abs(float(lps[b, 0]) - want_lp), float(score[want] - sg), margin, tol))
            assert abs(float(lps[b, 0]) - want_lp) <= tol and sg >= score[want] - tol
            assert g == want or margin < 2 * tol, (b, g, want, margin)


# ------------------------------------------------------------------------------------------------ 6. teacher-forced against the fp64 oracle
@pytest.mark.parametrize('name', list(R.SHAPES))
def test_generate_against_the_fp64_oracle(name):
    """cachegen_ref.check_margins on the rows the GPU drew: log-probs and perturbed-score margins within the position's tolerance,
    the fp64 token wherever the fp64 margin is twice that, at most 10 % near-ties (the CPU test pins the reference's own share on
    these inputs); one leg at the sharpest theta on the log-probs alone.  Prints the measured errors per leg."""
    case = R.oracle_case(name)
    cfg, params = case['cfg'], case['params']
    m = new_model(cfg, params=params)
    cache = m.cache_from(case['keys'], case['vals'])
    args = (params, cfg, case['keys'], case['vals'], R.GROUP)
    for theta in case['thetas'][:2]:
        for temperature, top_k in R.PICKS:
            toks, lps = m.cache_generate(cache, 5, R.NUM, theta, R.LAMBDA, group=R.GROUP, temperature=temperature, top_k=top_k,
                                         seed=R.SEED, primer=case['primer'], logprobs=True)
            res = R.check_margins(*args, theta, R.LAMBDA, toks, lps, temperature, top_k, R.SEED, primer=case['primer'])
            print('%s theta %.4g T %.1f top_k %d: log-prob error %.3g (tolerance there %.3g; %.3g .. %.3g), perturbed score at most '
                  '%.3g below the maximum, %d of %d positions near-ties' % (name, theta, temperature, top_k, res['lp_err'], res['lp_tol'],
                                                                            res['tol_min'], res['tol_max'], res['slack'], res['near'], res['total']))
            assert res['total'] == 5 * R.NUM and res['near'] <= 0.10 * res['total']
    # the sharpest theta: log-probs only
    theta = case['thetas'][2]
    toks, lps = m.cache_generate(cache, 5, R.NUM, theta, R.LAMBDA, group=R.GROUP, temperature=1.0, seed=R.SEED, primer=case['primer'],
                                 logprobs=True)
    res = R.check_margins(*args, theta, R.LAMBDA, toks, lps, 1.0, 0, R.SEED, primer=case['primer'], tokens=False)
    print('%s theta %.4g (log-probs only): error %.3g (tolerance there %.3g; %.3g .. %.3g)'
          % (name, theta, res['lp_err'], res['lp_tol'], res['tol_min'], res['tol_max']))
    cache.close()
    m.close()


# ------------------------------------------------------------------------------------------------ 7. plugin and errors
def test_plugin_generates_from_the_mixture(tmp_path):
    from models.cache_lstm import CacheLSTM
    from models.lstm_baseline import LSTMBaseline
    case = R.oracle_case('H24')
    theta, lam, T, P = case['thetas'][1], 0.25, 16, 8
    cfg = dict(case['cfg'], name='cache_lstm', checkpt_dir=str(tmp_path / 'cache'), cache_theta=theta, cache_lambda=lam)
    model = CacheLSTM(cfg)
    model.recover_or_init('')
    m = model.engine
    m.set_params({k: v.astype(np.float32) for k, v in case['params'].items()})
    support = case['support'].reshape(2, 3, T)
    # the default is the baseline's generate
    kw = dict(n=4, temperature=0.9, top_k=6, seed=3, primer_len=P, logprobs=True)
    base = LSTMBaseline.generate(model, support, T - P, **kw)
    plain = model.generate(support, T - P, **kw)
    assert np.array_equal(plain[0], base[0]) and _same(plain[1], base[1])
    # cache=True draws from the distribution fsmg_cache_score scores: the log-probs it reports for its own tokens are cache_score's
    toks, lps = model.generate(support, T - P, cache=True, **kw)
    assert not np.array_equal(toks, base[0])
    rows = np.concatenate([case['support'][np.arange(4) % 6, :P], toks], axis=1).astype(np.int32)
    cache = m.cache_build(case['support'], n_groups=1)
    sc = m.cache_score(cache, rows, [theta], [lam, 0.0], lstm_logprob=True)
    keys = cache.get()[0].astype(np.float64)
    cache.close()
    # both sides' hidden states are within the project's 2e-5 per unit of fp64: twice the oracle test's tolerance, |q_j| < 1
    tol = 2 * R.tolerance(theta, cfg['hidden_size'] + np.abs(keys[0]).sum(axis=1).max())
    err = float(np.abs(sc['logprob'][0, 0][:, P:].astype(np.float64) - lps).max())
    print('generate(cache=True) log-probs against cache_score of its rows: %.3g (tolerance %.3g)' % (err, tol))
    assert err <= tol
    assert float(np.abs(sc['logprob'][0, 1][:, P:].astype(np.float64) - lps).max()) > tol       # ... and not the model's alone
    # row 1 copies support song 1 up to the primer: the mixture cache=True draws from gives that song's continuation a higher mean
    # log-prob than the model cache=False draws from (the reference gains 1.5 nats here)
    copy = m.cache_build(case['support'], n_groups=1)
    song = m.cache_score(copy, case['support'][1:2], [theta], [lam], lstm_logprob=True)
    copy.close()
    mixed, alone = float(song['logprob'][0, 0, 0, P:].mean()), float(song['lstm_logprob'][0, P:].mean())
    print('the copied song\'s continuation: %.4f under the mixture, %.4f under the model' % (mixed, alone))
    assert mixed > alone + 0.5
    # with a decode state primed on the support songs
    cond = model.generate(support, 6, n=2, seed=5, cache=True, condition_on_support=True, primer_len=2)
    assert cond.shape == (2, 6) and np.array_equal(cond, model.generate(support, 6, n=2, seed=5, cache=True, condition_on_support=True,
                                                                        primer_len=2))
    assert model.sample(support[0], 5) == LSTMBaseline.sample(model, support[0], 5)


def test_argument_errors():
    from fsmg import binding as B
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m, m2 = new_model(cfg), new_model(cfg)
    lib = m._lib
    F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rng = np.random.RandomState(0)
    songs = rng.randint(0, 50, size=(4, 8)).astype(np.int32)
    cache, foreign = m.cache_build(songs, n_groups=2), m2.cache_build(songs, n_groups=2)
    big = m.cache_from(np.zeros((1, 1 << 16, 16), np.float32), np.zeros((1, 1 << 16), np.int32))
    st = m.new_state(3, history=16)
    # the destroyed cache is the last one made: a cache created after it could be given its address, and would then be that pointer
    gone = m.cache_build(songs, n_groups=2)
    gone_ptr = gone._c
    gone.close()
    st_before = st.get()
    toks, lps = np.full((1025, 4), -5, np.int32), np.full((1025, 4), 7.0, np.float32)
    q, z = np.zeros((1025, 16), np.float32), np.zeros((1025, 51), np.float32)
    outs = [np.full((1025, 51), 7.0, np.float32), np.full((1025, 51), 7.0, np.float32), np.full(1025, 7.0, np.float32)]

    def config(theta=1.0, lam=0.5, **over):
        c = m.cache_gen_config(theta, lam)
        for k, v in over.items():
            if k == 'reserved':
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return c

    def ptr(a, kind):
        return None if a is None else np.ascontiguousarray(a, np.int32 if kind is I32P else np.float32).ctypes.data_as(kind)

    def generate(c=None, cache_ptr=None, group=None, n_seq=3, primer=None, out=toks, state=False, gen=None, **over):
        g = m.gen_config(n_seq, 4, primer_len=0 if primer is None else primer.shape[1], **(gen or {}))
        pp = None if primer is None else C.c_void_p(primer.ctypes.data)
        head = (m._h, st._st) if state else (m._h,)
        tail = (ptr(group, I32P),) if state else (ptr(group, I32P), pp)
        fn = lib.fsmg_dstate_cache_generate if state else lib.fsmg_cache_generate
        return fn(*head, cache._c if cache_ptr is None else cache_ptr, C.byref(c or config(**over)), C.byref(g), None, *tail,
                  None if out is None else out.ctypes.data_as(I32P), lps.ctypes.data_as(F32P))

    def distribution(c=None, cache_ptr=None, group=None, n=3, qq=q, zz=z, o=(0, 1, 2), **over):
        o = [outs[i].ctypes.data_as(F32P) if i in o else None for i in range(3)]
        return lib.fsmg_cache_distribution(m._h, cache._c if cache_ptr is None else cache_ptr, C.byref(c or config(**over)), n,
                                           ptr(qq, F32P), ptr(zz, F32P), ptr(group, I32P), *o)

    calls = (generate, lambda **kw: generate(state=True, **kw), distribution)
    bad_everywhere = (dict(cache_ptr=foreign._c), dict(cache_ptr=gone_ptr), dict(cache_ptr=C.c_void_p()), dict(version=2),
                      dict(version=0), dict(reserved=0), dict(reserved=12), dict(theta=-0.5), dict(theta=float('nan')),
                      dict(theta=float('inf')), dict(lam=-0.01), dict(lam=1.01), dict(lam=float('nan')), dict(group=[0, 2, 0]),
                      dict(group=[0, -1, 0]))
    for call in calls:
        for kw in bad_everywhere:
            assert call(**kw) == -1, kw
            assert m._lib.fsmg_last_error(m._h), kw                         # ... with a message
    assert distribution(n=0) == -1 and distribution(n=(1 << 20) + 1) == -1
    assert distribution(o=()) == -1 and distribution(qq=None) == -1 and distribution(zz=None) == -1
    assert distribution(cache_ptr=big._c, n=1025) == -1                     # rows * Mg > 2^26
    assert generate(cache_ptr=big._c, n_seq=1025) == -1
    assert generate(n_seq=0) == -1 and generate(out=None) == -1             # what fsmg_generate refuses
    assert generate(gen=dict(temperature=-1.0)) == -1 and generate(gen=dict(top_k=52)) == -1
    assert generate(state=True, n_seq=4) == -1                              # what fsmg_dstate_generate refuses
    bad_primer = np.full((3, 2), 50, np.int32)
    assert generate(primer=bad_primer) == -7                                # FSMG_ERR_TOKEN_RANGE as fsmg_generate returns it
    # nothing was written, the state is what it was
    assert np.all(toks == -5) and np.all(lps == 7.0) and all(np.all(o == 7.0) for o in outs)
    after = st.get()
    assert all(_same(st_before[k], after[k]) for k in ('h', 'c', 'ctx')) and after['n_gen'] == 0 and after['n_ctx'] == 0
    # and the same calls are accepted when nothing is wrong
    assert generate() == 0 and generate(state=True) == 0 and distribution() == 0
    assert generate(group=[0, 1, 1]) == 0 and distribution(group=[1, 0, 1], o=(2,)) == 0
    assert distribution(cache_ptr=big._c, n=1024, o=(0,)) == 0              # rows * Mg = 2^26: the limit itself
    with pytest.raises(ValueError):
        m.cache_distribution(cache, np.zeros((2, 15), np.float32), np.zeros((2, 51), np.float32), 1.0, 0.5)
    with pytest.raises(ValueError):
        m.cache_generate(cache, 3, 4, 1.0, 0.5, group=[0, 1])
    with pytest.raises(B.FsmgError) as e:
        m.cache_generate(foreign, 3, 4, 1.0, 0.5)
    assert e.value.code == -1
    for c in (cache, foreign, big):
        c.close()
    st.close()
    m.close()
    m2.close()
