"""The fp64 restatement of the support-set cache's contract (tests/cache_ref.py) against a brute-force loop, the mixture's edge
cases, the layout of the config structs, and the argument checks of the binding and the C entry points that need no device.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cache_ref as R
from conftest import ROOT


def _case(seed, G, Mg, H, n, n_tokens=7):
    rng = np.random.RandomState(seed)
    keys = rng.normal(size=(G, Mg, H))
    vals = rng.randint(0, n_tokens, size=(G, Mg))
    q = rng.normal(size=(n, H))
    y = rng.randint(0, n_tokens + 1, size=n)                   # n_tokens itself occurs nowhere
    group = rng.randint(0, G, size=n)
    return keys, vals, q, y, group


def _brute(keys, vals, q, y, group, theta):
    out = []
    for qi, yi, g in zip(q, y, group):
        w = [math.exp(theta * (float(np.dot(qi, k)) - max(float(np.dot(qi, kk)) for kk in keys[g]))) for k in keys[g]]
        out.append(sum(wi for wi, v in zip(w, vals[g]) if v == yi) / sum(w))
    return np.array(out)


@pytest.mark.parametrize('G,Mg,H,n', [(1, 1, 3, 2), (2, 17, 5, 9), (3, 64, 24, 20)])
def test_vectorised_reference_against_brute_force(G, Mg, H, n):
    keys, vals, q, y, group = _case(0, G, Mg, H, n)
    thetas = [0.0, 0.7, 3.0]
    got = R.attend_groups(keys, vals, q, y, group, thetas)
    for k, th in enumerate(thetas):
        assert np.allclose(got[k], _brute(keys, vals, q, y, group, th), rtol=1e-12, atol=0)
    absent = y == 7
    assert absent.any() and np.all(got[:, absent] == 0.0)      # a target no entry holds: exactly 0
    assert np.allclose(got[0], [(vals[g] == yi).mean() for yi, g in zip(y, group)])     # theta = 0: the share of the hits
    one = R.attend(keys[0], vals[0], q, y, thetas)             # group None = all in group 0
    assert np.array_equal(one, R.attend_groups(keys, vals, q, y, None, thetas))


def test_fp32_mode_is_close_and_is_fp32():
    keys, vals, q, y, group = _case(1, 2, 65, 200, 33)
    p64 = R.attend_groups(keys, vals, q, y, group, [1.0])
    p32 = R.attend_groups(keys.astype(np.float32), vals, q.astype(np.float32), y, group, [1.0], np.float32)
    assert p32.dtype == np.float32
    pos = p64 > 0
    assert np.array_equal(p32 == 0, ~pos)
    assert (np.abs(p32[pos] - p64[pos]) / p64[pos]).max() < 1e-3   # inputs rounded to fp32 and scores of tens of units


def test_mixture_edge_cases():
    lp = np.log(np.array([0.5, 0.01, 1e-30, 0.2], np.float32))
    pc = np.array([0.25, 0.0, 0.5, 1.0], np.float32)
    assert np.array_equal(R.mix(lp, pc, 0.0).view(np.uint32), lp.view(np.uint32))              # lambda = 0: lp bitwise
    with np.errstate(divide='ignore'):
        assert np.array_equal(R.mix(lp, pc, 1.0), np.log(pc.astype(np.float64)).astype(np.float32))   # lambda = 1: log p_cache, -inf at 0
    got = R.mix(lp, pc, 0.25)
    want = np.log(0.75 * np.exp(lp.astype(np.float64)) + 0.25 * pc.astype(np.float64))
    assert np.allclose(got, want, rtol=1e-6, atol=0)
    assert got[1] == np.float32(math.log(0.75) + float(lp[1]))                                 # p_cache = 0: only the model's share
    assert R.mix(np.float32(-np.inf), np.float32(0.0), 0.5) == -np.inf
    assert R.mix(np.float32(-np.inf), np.float32(0.0), 1.0) == -np.inf


def test_entries_layout():
    hidden = np.arange(6 * 4 * 2, dtype=np.float64).reshape(6, 4, 2)
    songs = np.arange(24).reshape(6, 4)
    keys, vals = R.entries(hidden, songs, 2)
    assert keys.shape == (2, 12, 2) and vals.shape == (2, 12)
    for r in range(6):
        for t in range(4):
            g, e = r // 3, (r % 3) * 4 + t
            assert np.array_equal(keys[g, e], hidden[r, t]) and vals[g, e] == songs[r, t]


def test_config_layouts_match_the_header():
    from fsmg import binding as B
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert C.sizeof(B.FsmgCacheConfig) == 64 and C.sizeof(B.FsmgCacheScoreConfig) == 160
    assert [f[0] for f in B.FsmgCacheConfig._fields_] == ['version', 'n_rows', 'n_groups', 'tokens_on_device', 'pass_rows', 'reserved']
    assert [f[0] for f in B.FsmgCacheScoreConfig._fields_] == ['version', 'n_rows', 'tokens_on_device', 'nll_first', 'nll_count',
                                                                'pass_rows', 'n_theta', 'n_lambda', 'thetas', 'lambdas', 'reserved']
    for name in ('FSMG_CACHE_CONFIG_VERSION', 'FSMG_CACHE_SCORE_CONFIG_VERSION', 'FSMG_CACHE_MAX_THETA', 'FSMG_CACHE_MAX_LAMBDA'):
        assert int(re.search(r'#define %s (\d+)' % name, text).group(1)) == getattr(B, name)
    for struct, cls in (('fsmg_cache_config', B.FsmgCacheConfig), ('fsmg_cache_score_config', B.FsmgCacheScoreConfig)):
        body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), text, flags=re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        fields = re.findall(r'(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;', body)
        assert [(n, int(k or 1)) for _, n, k in fields] == [(n, C.sizeof(t) // 4) for n, t in cls._fields_]
    assert int(re.search(r'#define FSMG_CONFIG_VERSION (\d+)', text).group(1)) == B.FSMG_CONFIG_VERSION


def test_binding_refuses_bad_thetas_and_lambdas_without_a_device():
    from fsmg.binding import FsmgModel
    c = FsmgModel.cache_score_config(5, [0.0, 1.5], 0.25, nll_first=1, nll_count=2, pass_rows=3)
    assert (c.n_rows, c.n_theta, c.n_lambda, c.nll_first, c.nll_count, c.pass_rows) == (5, 2, 1, 1, 2, 3)
    assert list(c.thetas)[:2] == [0.0, 1.5] and c.lambdas[0] == 0.25 and not any(c.reserved)
    for thetas, lambdas in (([], [0.5]), ([1.0] * 9, [0.5]), ([-0.1], [0.5]), ([np.nan], [0.5]), ([np.inf], [0.5]),
                            ([1.0], []), ([1.0], [0.1] * 17), ([1.0], [-0.01]), ([1.0], [1.01]), ([1.0], [np.nan])):
        with pytest.raises(ValueError):
            FsmgModel.cache_score_config(5, thetas, lambdas)


def test_entry_points_are_declared_bound_exported_and_refuse_a_null_handle():
    from fsmg.build import build
    build()
    from fsmg import binding as B
    out = subprocess.check_output(['nm', '-D', '--defined-only', B.library_path()], universal_newlines=True)
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    names = ('fsmg_cache_build', 'fsmg_cache_create_from', 'fsmg_cache_get', 'fsmg_cache_info', 'fsmg_cache_destroy',
             'fsmg_cache_attend', 'fsmg_cache_score', 'fsmg_cache_eval_step')
    for name in names:
        assert name in B.SIGNATURES and re.search(r' T %s$' % name, out, flags=re.M) and re.search(r'\bint %s\(' % name, text), name
    assert 'k_cache_attend' in open(B.library_path(), 'rb').read().decode('latin-1')
    lib = B.load_library()
    assert lib.fsmg_version() == 600
    cb = B.FsmgCacheConfig(version=B.FSMG_CACHE_CONFIG_VERSION, n_rows=2, n_groups=1)
    cs = B.FsmgModel.cache_score_config(2, [1.0], [0.5])
    toks = np.zeros((2, 4), np.int32)
    f = np.zeros(64, np.float32)
    i = np.zeros(8, np.int32)
    out_p, info, nll = C.c_void_p(), (C.c_int64 * 4)(), C.c_float()
    tp, fp, ip = C.c_void_p(toks.ctypes.data), f.ctypes.data_as(C.POINTER(C.c_float)), i.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.fsmg_cache_build(None, C.byref(cb), tp, C.byref(out_p)) == -1
    assert lib.fsmg_cache_create_from(None, 1, 2, fp, ip, C.byref(out_p)) == -1
    assert lib.fsmg_cache_get(None, None, fp, ip) == -1
    assert lib.fsmg_cache_info(None, None, info) == -1
    assert lib.fsmg_cache_destroy(None, None) == -1
    assert lib.fsmg_cache_attend(None, None, 1, fp, ip, None, fp, 1, fp) == -1
    assert lib.fsmg_cache_score(None, None, C.byref(cs), tp, None, fp, None, None, None) == -1
    assert lib.fsmg_cache_eval_step(None, tp, tp, 1, 1, 1, 1.0, 0.5, C.byref(nll)) == -1


def test_plugin_config_checks_need_no_device():
    from models.cache_lstm import CacheLSTM
    from conftest import small_config
    for over in (dict(), dict(cache_theta=1.0), dict(cache_lambda=0.5), dict(cache_theta=-1.0, cache_lambda=0.5),
                 dict(cache_theta=1.0, cache_lambda=1.5), dict(cache_theta=float('nan'), cache_lambda=0.5)):
        with pytest.raises(RuntimeError, match='cache_'):
            CacheLSTM(dict(small_config(), **over))
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'cache_lstm.yaml')))
    base = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'lstm_baseline.yaml')))
    assert cfg['model_module_name'] == 'models.cache_lstm' and cfg['model_class_name'] == 'CacheLSTM'
    assert cfg['cache_theta'] >= 0 and 0 <= cfg['cache_lambda'] <= 1
    assert {k: v for k, v in cfg.items() if k not in ('name', 'model_module_name', 'model_class_name', 'cache_theta', 'cache_lambda')} == \
           {k: v for k, v in base.items() if k not in ('name', 'model_module_name', 'model_class_name')}
