"""The fp64 restatement of cache-conditioned generation (tests/cachegen_ref.py) against a brute-force loop, its decoder against
gen_ref's, the near-tie share of the inputs the teacher-forced GPU test uses, the layout of the config struct, and what the binding
and the C entry points refuse without a device.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cachegen_ref as R
import gen_ref as G
from conftest import ROOT, small_config
from oracle import lstm_oracle as O


def _brute(keys, vals, q, z, group, theta, lam):
    """every entry and every column in a loop: -> p_cache [n, V1], z'' [n, V1]"""
    n, V1 = z.shape
    pc, zz = np.zeros((n, V1)), np.zeros((n, V1))
    for i in range(n):
        g = group[i]
        d = [float(np.dot(q[i], k)) for k in keys[g]]
        w = [math.exp(theta * (x - max(d))) for x in d]
        lse = max(z[i]) + math.log(sum(math.exp(x - max(z[i])) for x in z[i]))
        for v in range(V1):
            mass = [wi for wi, vi in zip(w, vals[g]) if vi == v]
            pc[i, v] = sum(mass) / sum(w) if mass else 0.0
            a = (math.log1p(-lam) if lam < 1 else -math.inf) + (z[i, v] - lse)
            b = math.log(lam) + math.log(pc[i, v]) if lam > 0 and pc[i, v] > 0 else -math.inf
            hi, lo = max(a, b), min(a, b)
            zz[i, v] = hi if lo == -math.inf else hi + math.log1p(math.exp(lo - hi))
    return pc, zz


@pytest.mark.parametrize('G_,Mg,H,n,V1', [(1, 1, 3, 2, 5), (2, 17, 5, 9, 12), (3, 64, 24, 20, 30)])
def test_distribution_against_brute_force(G_, Mg, H, n, V1):
    rng = np.random.RandomState(0)
    keys, q, z = rng.normal(size=(G_, Mg, H)), rng.normal(size=(n, H)), rng.normal(size=(n, V1)) * 2
    vals = rng.randint(0, max(V1 - 2, 1), size=(G_, Mg))           # the last columns occur nowhere
    group = rng.randint(0, G_, size=n)
    for theta in (0.0, 0.7, 3.0):
        for lam in (0.0, 0.25, 1.0):
            got = R.distribution(keys, vals, q, z, group, theta, lam)
            pc, zz = _brute(keys, vals, q, z, group, theta, lam)
            assert np.allclose(got['cache_prob'], pc, rtol=1e-12, atol=0)
            assert np.array_equal(got['cache_prob'] == 0, pc == 0) and np.all(got['cache_prob'][:, V1 - 1] == 0)
            assert np.allclose(got['cache_prob'].sum(axis=1), 1.0, rtol=1e-12)
            fin = np.isfinite(zz)
            assert np.array_equal(np.isfinite(got['logprob']), fin) and np.allclose(got['logprob'][fin], zz[fin], rtol=1e-12, atol=1e-12)
            if lam == 0.0:
                assert np.array_equal(got['logprob'], got['lp'])
            if lam == 1.0:
                assert np.all(got['logprob'][pc == 0] == -np.inf)
            assert np.allclose(np.exp(got['logprob']).sum(axis=1), 1.0, rtol=1e-12)       # the mixture is a distribution
    none = R.distribution(keys, vals, q, z, None, 0.7, 0.25)
    assert np.array_equal(none['cache_prob'], R.distribution(keys, vals, q, z, np.zeros(n, int), 0.7, 0.25)['cache_prob'])
    p64 = R.distribution(keys, vals, q, z, group, 0.7, 0.25)['cache_prob']
    p32 = R.distribution(keys.astype(np.float32), vals, q.astype(np.float32), z, group, 0.7, 0.25, np.float32)['cache_prob']
    assert p32.dtype == np.float32 and np.array_equal(p32 == 0, p64 == 0) and np.allclose(p32, p64, rtol=1e-3, atol=0)


def _small():
    cfg = small_config(input_size=30, max_len=8, embedding_size=6, hidden_size=10, n_layers=2)
    params = O.glorot_init(cfg, 3)
    rng = np.random.RandomState(4)
    keys = rng.normal(size=(2, 20, 10)) * 0.5
    vals = np.stack([rng.randint(0, 10, size=20), rng.randint(10, 20, size=20)])       # the groups' values are disjoint
    return cfg, params, keys, vals


def test_reference_decoder_extends_gen_ref():
    cfg, params, keys, vals = _small()
    group = np.array([0, 1, 0])
    primer = np.array([[1, 2], [3, 4], [5, 6]])
    # lambda = 0: gen_ref's decoder
    a = R.generate(params, cfg, keys, vals, group, 2.0, 0.0, 3, 6, temperature=0.9, top_k=4, seed=5, primer=primer)
    toks, lps = G.generate(params, cfg, 3, 6, temperature=0.9, top_k=4, seed=5, primer=primer)
    assert np.array_equal(a['toks'], toks) and np.allclose(a['lps'], lps, rtol=0, atol=1e-12)
    # lambda = 1: every token is a value of the row's own group
    b = R.generate(params, cfg, keys, vals, group, 2.0, 1.0, 3, 6, seed=5)
    for r in range(3):
        assert set(b['toks'][r]) <= set(vals[group[r]])
    # the check accepts the reference's own draw with nothing to spare, and refuses a changed token and a shifted log-prob
    c = R.generate(params, cfg, keys, vals, group, 2.0, 0.25, 3, 6, temperature=0.8, top_k=5, seed=9, primer=primer)
    args = (params, cfg, keys, vals, group, 2.0, 0.25)
    res = R.check_margins(*args, c['toks'], c['lps'], 0.8, 5, 9, primer=primer)
    assert res['total'] == 18 and res['lp_err'] <= 1e-12 and res['slack'] <= 1e-12
    assert res['near'] == int((c['margin'] < 2 * c['tol']).sum())
    assert np.all(c['tol'] >= 1e-4) and res['tol_min'] == c['tol'].min() and res['tol_max'] == c['tol'].max()
    sure = np.argwhere(c['margin'] >= 1.0)
    assert len(sure)
    r, t = sure[-1]
    wrong = c['toks'].copy()
    wrong[r, t] = (wrong[r, t] + 1) % 30
    with pytest.raises(AssertionError):
        R.check_margins(*args, wrong, c['lps'], 0.8, 5, 9, primer=primer, rows=[r])
    with pytest.raises(AssertionError, match='logprob'):
        R.check_margins(*args, c['toks'], c['lps'] + 0.01, 0.8, 5, 9, primer=primer)
    R.check_margins(*args, c['toks'], c['lps'], 0.8, 5, 10, primer=primer, tokens=False)     # log-probs only: the seed is not read


@pytest.mark.parametrize('name', list(R.SHAPES))
def test_near_tie_share_of_the_gpu_tests_inputs(name):
    """On the reference alone: the free-running fp64 draw over the teacher-forced GPU test's shapes, thetas, picks and seed leaves
    at most 10 % of the generated positions with an fp64 margin below the tie threshold (twice the position's tolerance), so the GPU
    test's cap on skipped positions is one the inputs can meet."""
    case = R.oracle_case(name)
    for theta in case['thetas'][:2]:
        for temperature, top_k in R.PICKS:
            out = R.generate(case['params'], case['cfg'], case['keys'], case['vals'], R.GROUP, theta, R.LAMBDA, 5, R.NUM,
                             temperature=temperature, top_k=top_k, seed=R.SEED, primer=case['primer'])
            share = float((out['margin'] < 2 * out['tol']).mean())
            print('%s theta %.4g T %.1f top_k %d: near-tie share %.3f (tolerance %.3g .. %.3g, smallest margin %.3g)'
                  % (name, theta, temperature, top_k, share, out['tol'].min(), out['tol'].max(), out['margin'].min()))
            assert share <= 0.10
            # the cache is felt: some drawn tokens are values of the row's group
            assert any(t in set(case['vals'][R.GROUP[b]]) for b in range(5) for t in out['toks'][b])


def test_config_layout_matches_the_header():
    from fsmg import binding as B
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert C.sizeof(B.FsmgCacheGenConfig) == 64
    for name in ('FSMG_CACHE_GEN_CONFIG_VERSION', 'FSMG_CACHE_GEN_CHUNK'):
        assert int(re.search(r'#define %s (\d+)' % name, text).group(1)) == getattr(B, name)
    body = re.search(r'typedef struct fsmg_cache_gen_config \{(.*?)\} fsmg_cache_gen_config;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;', body)
    assert [(n, int(k or 1)) for _, n, k in fields] == [(n.rstrip('_'), C.sizeof(t) // 4) for n, t in B.FsmgCacheGenConfig._fields_]
    c = B.FsmgModel.cache_gen_config(1.5, 0.25)
    assert (c.version, c.theta, c.lambda_) == (1, 1.5, 0.25) and not any(c.reserved)
    kernels = open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'csrc', 'fsmg_kernels.h')).read()
    assert int(re.search(r'constexpr int CACHE_GEN_CHUNK = (\d+);', kernels).group(1)) == B.FSMG_CACHE_GEN_CHUNK


def test_entry_points_are_declared_bound_exported_and_refuse_a_null_handle():
    from fsmg.build import build
    build()
    from fsmg import binding as B
    out = subprocess.check_output(['nm', '-D', '--defined-only', B.library_path()], universal_newlines=True)
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    for name in ('fsmg_cache_generate', 'fsmg_dstate_cache_generate', 'fsmg_cache_distribution'):
        assert name in B.SIGNATURES and re.search(r' T %s$' % name, out, flags=re.M) and re.search(r'\bint %s\(' % name, text), name
    blob = open(B.library_path(), 'rb').read().decode('latin-1')
    assert 'k_cache_scores' in blob and 'k_cache_mix' in blob
    lib = B.load_library()
    cc = B.FsmgModel.cache_gen_config(1.0, 0.5)
    gc = B.FsmgModel.gen_config(2, 3)
    f = np.zeros(64, np.float32)
    i = np.zeros(8, np.int32)
    fp, ip = f.ctypes.data_as(C.POINTER(C.c_float)), i.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.fsmg_cache_generate(None, None, C.byref(cc), C.byref(gc), None, None, None, ip, fp) == -1
    assert lib.fsmg_dstate_cache_generate(None, None, None, C.byref(cc), C.byref(gc), None, None, ip, fp) == -1
    assert lib.fsmg_cache_distribution(None, None, C.byref(cc), 1, fp, fp, None, fp, fp, fp) == -1
    assert np.all(f == 0) and np.all(i == 0)


class _FakeEngine(object):
    """stands in for FsmgModel under the plugin: records what CacheLSTM.generate asks of it"""

    def __init__(self):
        self.calls = []

    def generate(self, n_seq, num, **kw):
        self.calls.append(('generate', n_seq, num, kw))
        return np.zeros((n_seq, num), np.int32)

    def cache_build(self, songs, n_groups=1):
        self.calls.append(('cache_build', np.asarray(songs).shape, n_groups))
        engine = self

        class _Cache(object):
            def close(self):
                engine.calls.append(('close',))
        return _Cache()

    def cache_generate(self, cache, n_seq, num, theta, lam, **kw):
        self.calls.append(('cache_generate', n_seq, num, theta, lam, kw))
        return np.ones((n_seq, num), np.int32)


def test_plugin_routes_generate_through_the_cache_only_on_request():
    from models.cache_lstm import CacheLSTM
    model = CacheLSTM.__new__(CacheLSTM)
    model._theta, model._lambda, model._time_steps, model._start_word = 1.5, 0.25, 4, 9
    model._model, model._require_init = _FakeEngine(), lambda: None
    support = np.arange(24).reshape(2, 3, 4) % 9
    assert np.all(model.generate(support, 5, n=2, temperature=0.5, primer_len=2) == 0)
    name, n_seq, num, kw = model._model.calls[-1]
    assert (name, n_seq, num, kw['temperature']) == ('generate', 2, 5, 0.5) and np.array_equal(kw['primer'], support.reshape(6, 4)[:2, :2])
    del model._model.calls[:]
    assert np.all(model.generate(support, 5, n=2, cache=True, top_k=3, primer_len=2) == 1)
    calls = model._model.calls
    assert calls[0] == ('cache_build', (6, 4), 1) and calls[-1] == ('close',)
    name, n_seq, num, theta, lam, kw = calls[1]
    assert (name, n_seq, num, theta, lam, kw['top_k']) == ('cache_generate', 2, 5, 1.5, 0.25, 3)
    assert np.array_equal(kw['primer'], support.reshape(6, 4)[:2, :2]) and 'state' not in kw
