"""The decode-time self-cache (fsmg_cache_self_distribution / fsmg_cache_self_generate) on the MI355X against the fp64 restatement
(tests/selfcache_ref.py): the union's whole distribution at the window, chunk and support edges with duplicated values, the bitwise
promises of generation, its log-probs against fsmg_cache_self_score, and the decoder teacher-forced against the fp64 oracle.

Tolerances: p_cache within max(8 e32, 1e-6) of fp64 (e32 the restatement in fp32 on the same inputs), relative where
fp64 > 0 and exactly 0 where it is 0; log-probs within 1e-4 + theta 2e-5 l1 over the entries the position sees."""
import ctypes as C
import functools

import numpy as np
import pytest

import cache_ref as CR
import selfcache_ref as SC
from conftest import small_config
from gpu_utils import new_model

pytestmark = pytest.mark.gpu

START = 97
PALETTE = np.array([0, 3, 5, 11, 42, 96, START], np.int32)     # few values: duplicates among the own entries; 50 occurs nowhere


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _rel_err(got, want64):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    pos = want64 > 0
    assert np.all(got[~pos] == 0.0), 'a column no visible entry holds must give exactly 0'
    return float((np.abs(got[pos] - want64[pos]) / want64[pos]).max()) if pos.any() else 0.0


def _ulp_close(got, want32):
    got, want32 = np.asarray(got, np.float32), np.asarray(want32, np.float32)
    fin = np.isfinite(want32)
    return np.array_equal(got[~fin], want32[~fin]) and np.all(np.abs(got[fin].astype(np.float64) - want32[fin]) <= np.spacing(np.abs(want32[fin])))


@functools.lru_cache(maxsize=None)
def _dist_model(H):
    return new_model(small_config(input_size=START, max_len=4, embedding_size=8, hidden_size=H))


def _vectors(rng, shape):
    H = shape[-1]
    return (rng.normal(size=shape) * np.sqrt(3.0 / np.sqrt(H))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1. the distribution
@pytest.mark.parametrize('H', [24, 200, 512])
def test_self_distribution_against_fp64_at_the_edges(H):
    m = _dist_model(H)
    V1 = START + 1
    S = 33
    self_len = np.array([0, 1, 17, 16, 33, 15], np.int32)
    n = len(self_len)
    worst = (0.0, 0.0, '')
    for Mg in (0, 1, 17, 65):
        rng = np.random.RandomState(10 * H + Mg)
        keys = _vectors(rng, (2, Mg, H)) if Mg else None
        vals = PALETTE[rng.randint(0, len(PALETTE), size=(2, Mg))].astype(np.int32) if Mg else None
        group = np.array([0, 1, 1, 0, 1, 0], np.int32)
        cache = m.cache_from(keys, vals) if Mg else None
        q = _vectors(rng, (n, H))
        z = rng.normal(size=(n, V1)).astype(np.float32) * 2
        sk = _vectors(rng, (n, S, H))
        sv = PALETTE[rng.randint(0, len(PALETTE), size=(n, S))].astype(np.int32)       # duplicated values among the own entries
        if Mg:
            sv[2, 16] = vals[group[2], 0]                                               # a value a support AND an own entry hold
        d = np.concatenate([q.astype(np.float64).dot(sk[i].astype(np.float64).T) for i in range(n)])
        spread = float(d.max() - d.min())
        for W in (1, 15, 16, 17, 1000):
            for theta in (0.0, float(np.float32(5.0 / spread)), float(np.float32(40.0 / spread))):
                tag = 'H %d Mg %d W %d theta %.3g' % (H, Mg, W, theta)
                ref_kw = dict(keys=keys, vals=vals, group=group) if Mg else {}
                want = SC.distribution(q, z, sk, sv, self_len, W, theta, 0.25, **ref_kw)
                w32 = SC.distribution(q, z, sk, sv, self_len, W, theta, 0.25, dtype=np.float32, **ref_kw)
                got = m.cache_self_distribution(q, z, sk, sv, self_len, theta, 0.25, W, cache=cache, group=group if Mg else None)
                e32, err = _rel_err(w32['cache_prob'], want['cache_prob']), _rel_err(got['cache_prob'], want['cache_prob'])
                worst = max(worst, (err, e32, tag))
                assert err <= max(8 * e32, 1e-6), (tag, err, e32)
                sums = got['cache_prob'].astype(np.float64).sum(axis=1)
                for i in range(n):
                    if Mg == 0 and self_len[i] == 0:
                        assert np.all(got['cache_prob'][i] == 0.0), tag                 # the empty union
                    else:
                        assert abs(sums[i] - 1.0) <= 1e-6, (tag, i, sums[i])
                assert np.all(got['cache_prob'][:, 50] == 0.0)
                assert np.all(np.abs(got['lse'] - want['lse']) <= 4 * np.spacing(np.abs(want['lse']).astype(np.float32)))
                lp32 = z - got['lse'][:, None]                                          # fl32(z - lse) from the returned pieces
                for lam in (0.0, 0.25, 1.0):
                    g2 = got if lam == 0.25 else m.cache_self_distribution(q, z, sk, sv, self_len, theta, lam, W, cache=cache,
                                                                           group=group if Mg else None)
                    empty = (self_len == 0)[:, None] & (Mg == 0)
                    assert _ulp_close(g2['logprob'], SC.mix(lp32, g2['cache_prob'], lam, empty)), (tag, lam)
                    assert _same(g2['cache_prob'], got['cache_prob'])
                    if lam == 0.0:
                        assert _same(g2['logprob'], lp32), tag                          # lambda = 0: lp bitwise
                    if Mg == 0:
                        assert _same(g2['logprob'][0], lp32[0]), (tag, lam)             # the empty union: lp at every lambda
        # a row alone gives the bits it gives among the others
        one = m.cache_self_distribution(q[2:3], z[2:3], sk[2:3], sv[2:3], self_len[2:3], theta, 0.25, 17, cache=cache,
                                        group=group[2:3] if Mg else None)
        all_ = m.cache_self_distribution(q, z, sk, sv, self_len, theta, 0.25, 17, cache=cache, group=group if Mg else None)
        assert _same(one['logprob'][0], all_['logprob'][2]) and _same(one['cache_prob'][0], all_['cache_prob'][2])
        if cache is not None:
            cache.close()
    print('H %d: largest p_cache error %.3g (e32 there %.3g) at %s' % ((H,) + worst))


# ------------------------------------------------------------------------------------------------ 2. generate: the bitwise promises
@functools.lru_cache(maxsize=None)
def _gen_case(name):
    case = SC.oracle_case(name)
    m = new_model(case['cfg'], params=case['params'])
    return case, m


def test_generate_bitwise_promises():
    case, m = _gen_case('H24')
    cfg, primer = case['cfg'], case['primer']
    cache = m.cache_from(case['keys'], case['vals'])
    theta = case['thetas'][1]
    before = {k: v.copy() for k, v in m.get_params().items()}
    step0 = m.get_step() if hasattr(m, 'get_step') else None
    for c in (None, cache):
        kw = dict(cache=c, group=SC.GROUP if c is not None else None)
        # lambda = 0: generate() bitwise, with and without filters
        for filt in (dict(), dict(top_p=0.9, repetition_penalty=1.2, repeat_window=4)):
            a = m.cache_self_generate(5, 8, theta, 0.0, 6, temperature=0.8, top_k=7, seed=3, primer=primer, logprobs=True, **filt, **kw)
            b = m.generate(5, 8, temperature=0.8, top_k=7, seed=3, primer=primer, logprobs=True, **filt)
            assert _same(a[0], b[0]) and _same(a[1], b[1])
        # determinism; independence of n_seq
        a = m.cache_self_generate(5, 10, theta, 0.25, 6, temperature=0.9, seed=5, primer=primer, logprobs=True, **kw)
        b = m.cache_self_generate(5, 10, theta, 0.25, 6, temperature=0.9, seed=5, primer=primer, logprobs=True, **kw)
        assert _same(a[0], b[0]) and _same(a[1], b[1])
        kw3 = dict(cache=c, group=SC.GROUP[:3] if c is not None else None)
        s = m.cache_self_generate(3, 10, theta, 0.25, 6, temperature=0.9, seed=5, primer=primer[:3], logprobs=True, **kw3)
        assert _same(s[0], a[0][:3]) and _same(s[1], a[1][:3])
        assert not _same(a[0], m.generate(5, 10, temperature=0.9, seed=5, primer=primer))      # the cache is felt
    # lambda = 1 without support entries: every token after position 0 is a token already in the row (the primer counts)
    for P in (0, 3):
        pr = primer if P else None
        toks = m.cache_self_generate(5, 12, theta, 1.0, 6, temperature=1.0, seed=9, primer=pr)
        for b in range(5):
            row = ([int(w) for w in primer[b]] if P else []) + [int(w) for w in toks[b]]
            assert all(row[i] in row[:i] for i in range(max(P, 1), len(row))), (P, b, row)
    after = m.get_params()
    assert all(_same(before[k], after[k]) for k in before)                                     # handle state untouched
    if step0 is not None:
        assert m.get_step() == step0
    cache.close()


@pytest.mark.parametrize('name', ['H24', 'H200x2'])
def test_generate_logprobs_against_cache_self_score(name):
    """the log-probs generation reports for its own tokens against fsmg_cache_self_score on the generated rows padded to max_len
    (primer_len + num <= max_len), within the oracle bound of the position (the two paths run different recurrence kernels)"""
    case, m = _gen_case(name)
    cfg, primer = case['cfg'], case['primer']
    T, P, num, W = cfg['max_len'], 3, 10, 6
    cache = m.cache_from(case['keys'], case['vals'])
    hq_all = None
    for c in (None, cache):
        for theta in case['thetas'][:2]:
            toks, lps = m.cache_self_generate(5, num, theta, 0.25, W, cache=c, group=SC.GROUP if c is not None else None, temperature=1.0,
                                              seed=4, primer=primer, logprobs=True)
            rows = np.zeros((5, T), np.int32)
            rows[:, :P], rows[:, P:P + num] = primer, toks
            sc = m.cache_self_score(rows, [theta], [0.25], W, cache=c, group=SC.GROUP if c is not None else None)['logprob'][0, 0]
            ref = SC.score(case['params'], rows, W, [theta], [0.25], cfg, support=case['support'] if c is not None else None, n_groups=2,
                           group=SC.GROUP if c is not None else None)
            err = 0.0
            for b in range(5):
                for t in range(num):
                    p = P + t
                    k, _ = SC.union_entries(ref['queries'][b], rows[b], p, W, ref['keys'][SC.GROUP[b]] if c is not None else None,
                                            ref['values'][SC.GROUP[b]] if c is not None else None)
                    tol = SC._visible_tol(theta, ref['queries'][b, p], k)
                    e = abs(float(lps[b, t]) - float(sc[b, p]))
                    err = max(err, e)
                    assert e <= tol, (b, t, lps[b, t], sc[b, p], tol)
            print('%s support %d theta %.4g: generate against cache_self_score, largest difference %.3g' % (name, c is not None, theta, err))
    cache.close()


# ------------------------------------------------------------------------------------------------ 3. teacher-forced against the fp64 oracle
@pytest.mark.parametrize('name', ['H24', 'H200x2', 'H512'])
def test_generate_against_the_fp64_oracle(name):
    """selfcache_ref.check_margins on the rows the GPU drew, at most 10 % near-ties (the CPU test pins the reference's own count on
    these inputs at 5 % or less)"""
    case, m = _gen_case(name)
    cfg, params, primer = case['cfg'], case['params'], case['primer']
    cache = m.cache_from(case['keys'], case['vals'])
    for c in (None, cache):
        kw = dict(keys=case['keys'], vals=case['vals'], group=SC.GROUP) if c is not None else {}
        for theta in case['thetas'][:2]:
            for temperature, top_k in SC.GEN_PICKS:
                toks, lps = m.cache_self_generate(5, SC.GEN_NUM, theta, SC.GAIN_LAMBDA, SC.GEN_W, cache=c,
                                                  group=SC.GROUP if c is not None else None, temperature=temperature, top_k=top_k,
                                                  seed=SC.GEN_SEED, primer=primer, logprobs=True)
                res = SC.check_margins(params, cfg, SC.GEN_W, theta, SC.GAIN_LAMBDA, toks, lps, temperature, top_k, SC.GEN_SEED,
                                       primer=primer, **kw)
                ref = SC.generate(params, cfg, SC.GEN_W, theta, SC.GAIN_LAMBDA, 5, SC.GEN_NUM, temperature=temperature, top_k=top_k,
                                  seed=SC.GEN_SEED, primer=primer, **kw)
                print('%s support %d theta %.4g T %.1f top_k %d: log-prob error %.3g (tolerance there %.3g; %.3g .. %.3g), perturbed score at '
                      'most %.3g below the maximum, %d of %d positions near-ties on the GPU rows, %d on the reference alone'
                      % (name, c is not None, theta, temperature, top_k, res['lp_err'], res['lp_tol'], res['tol_min'], res['tol_max'],
                         res['slack'], res['near'], res['total'], int((ref['margin'] < 2 * ref['tol']).sum())))
                assert res['total'] == 5 * SC.GEN_NUM and res['near'] <= 0.10 * res['total']
    cache.close()


# ------------------------------------------------------------------------------------------------ 4. the plugin
def test_plugin_generates_from_the_union(tmp_path):
    from models.cache_lstm import CacheLSTM
    case = SC.oracle_case('H24')
    theta, T = case['thetas'][1], 16
    base = dict(case['cfg'], name='cache_lstm', cache_theta=theta, cache_lambda=0.25)
    plain = CacheLSTM(dict(base, checkpt_dir=str(tmp_path / 'plain')))
    both = CacheLSTM(dict(base, checkpt_dir=str(tmp_path / 'both'), cache_self=True, cache_window=6))
    for model in (plain, both):
        model.recover_or_init('')
        model.engine.set_params({k: np.asarray(v, np.float32) for k, v in case['params'].items()})
    support = case['support'].reshape(2, 3, T)
    m = both.engine
    kw = dict(temperature=0.9, seed=3, primer_len=3, logprobs=True)
    # cache=True with cache_self set: the union over one group built from the whole support set
    got = both.generate(support, 8, n=4, cache=True, **kw)
    primer = case['support'][np.arange(4) % 6, :3]
    one = m.cache_build(case['support'], n_groups=1)
    want = m.cache_self_generate(4, 8, theta, 0.25, 6, cache=one, temperature=0.9, seed=3, primer=primer, logprobs=True)
    sup_only = m.cache_generate(one, 4, 8, theta, 0.25, temperature=0.9, seed=3, primer=primer, logprobs=True)
    one.close()
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    # cache_self unset: cache=True is what it was; self_cache=True adds the own history, alone or beside the support set
    old = plain.generate(support, 8, n=4, cache=True, **kw)
    assert _same(old[0], sup_only[0]) and _same(old[1], sup_only[1])
    alone = plain.generate(support, 8, n=4, self_cache=True, **kw)
    want = plain.engine.cache_self_generate(4, 8, theta, 0.25, T, temperature=0.9, seed=3, primer=primer, logprobs=True)
    assert _same(alone[0], want[0]) and _same(alone[1], want[1])
    # an empty support set: nothing to prime from, nothing to build
    empty = plain.generate(np.zeros((0, T), np.int32), 8, n=3, self_cache=True, temperature=0.9, seed=3)
    assert _same(empty, plain.engine.cache_self_generate(3, 8, theta, 0.25, T, temperature=0.9, seed=3))
    base_draw = plain.generate(support, 8, n=4, **kw)
    assert _same(base_draw[0], plain.engine.generate(4, 8, temperature=0.9, seed=3, primer=primer, logprobs=True)[0])
    with pytest.raises(ValueError):
        both.generate(support, 8, n=4, cache=True, condition_on_support=True)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_argument_errors():
    from fsmg import binding as B
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    lib = m._lib
    F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    SENT = np.float32(-123.5)
    n, S, V1 = 2, 3, 51
    q, z = np.zeros((n, 16), np.float32), np.zeros((n, V1), np.float32)
    sk, sv, sl = np.zeros((n, S, 16), np.float32), np.zeros((n, S), np.int32), np.array([1, 3], np.int32)
    out = np.full((n, V1), SENT, np.float32)
    toks = np.full((2, 4), -77, np.int32)

    def dist(values=sv, lens=sl, n_=n, S_=S, theta=1.0, lam=0.5, out_=out, **over):
        cc, sc = m.cache_gen_config(theta, lam), m.cache_self_config(2)
        for k, v in over.items():
            if k == 'reserved':
                sc.reserved[v] = 1
            else:
                setattr(sc, k, v)
        out[...] = SENT
        rc = lib.fsmg_cache_self_distribution(m._h, None, C.byref(cc), C.byref(sc), n_, q.ctypes.data_as(F32P), z.ctypes.data_as(F32P),
                                              sk.ctypes.data_as(F32P), values.ctypes.data_as(I32P), lens.ctypes.data_as(I32P), S_, None,
                                              None, None if out_ is None else out_.ctypes.data_as(F32P), None)
        if rc != 0:
            assert lib.fsmg_last_error(m._h) and np.all(out == SENT)
        return rc

    def gen(num=4, primer_len=0, theta=1.0, lam=0.5, n_seq=2, **over):
        cc, sc = m.cache_gen_config(theta, lam), m.cache_self_config(2)
        for k, v in over.items():
            if k == 'reserved':
                sc.reserved[v] = 1
            else:
                setattr(sc, k, v)
        gc = m.gen_config(n_seq, num, 1.0, 0, 0, primer_len, 0)
        toks[...] = -77
        pr = np.zeros((2, max(primer_len, 1)), np.int32)
        rc = lib.fsmg_cache_self_generate(m._h, None, C.byref(cc), C.byref(sc), C.byref(gc), None, None,
                                          C.c_void_p(pr.ctypes.data) if primer_len else None, toks.ctypes.data_as(I32P), None)
        if rc != 0:
            assert lib.fsmg_last_error(m._h) and np.all(toks == -77)
        return rc

    assert dist() == 0 and not np.any(out == SENT) and gen() == 0 and np.all(toks >= 0)
    assert dist(version=2) == -1 and dist(reserved=3) == -1 and dist(window=0) == -1
    assert gen(version=0) == -1 and gen(reserved=13) == -1 and gen(window=-1) == -1
    assert dist(theta=-1.0) == -1 and dist(lam=1.5) == -1 and gen(theta=float('nan')) == -1 and gen(lam=-0.1) == -1
    assert dist(lens=np.array([1, 4], np.int32)) == -1 and dist(lens=np.array([-1, 0], np.int32)) == -1         # self_len outside [0, S]
    assert dist(n_=0) == -1 and dist(out_=None) == -1 and dist(S_=-1) == -1
    bad = sv.copy()
    bad[1, 2] = 52
    assert dist(values=bad) == -7
    assert gen(n_seq=1 << 20, num=40) == -1                                  # rows * (primer_len + num) * Hp = 2^20 * 40 * 16 > 2^29
    assert gen(num=-1) == -1
    assert dist(S_=0, lens=np.zeros(2, np.int32)) == 0                       # no own entries at all: the model alone
    assert np.allclose(out, -np.log(V1), atol=1e-6)
    m.close()
