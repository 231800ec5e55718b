"""The fp64 restatement of the self-cache's contract (tests/selfcache_ref.py) against a brute-force triple loop and against
cache_ref.attend over explicit entry lists, the empty-set rule, the copied-half song's gain on the fp64 oracle (the reference number of
the GPU test), the layout of the config struct and the entry points' refusals that need no device.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cache_ref as R
import selfcache_ref as SC
from conftest import ROOT


def _case(seed, T, H, Mg, n_tokens=5):
    rng = np.random.RandomState(seed)
    vec = rng.normal(size=(T, H))
    val = rng.randint(0, n_tokens, size=T)
    keys = rng.normal(size=(Mg, H)) if Mg else None
    vals = rng.randint(0, n_tokens + 1, size=Mg) if Mg else None
    return vec, val, keys, vals


def _brute(vec, val, W, theta, keys, vals):
    """the triple loop over (position, entry, column)"""
    T, H = vec.shape
    out = []
    for t in range(T):
        ents = [] if keys is None else [(keys[j], int(vals[j])) for j in range(len(vals))]
        ents += [(vec[i], int(val[i])) for i in range(T) if t - W <= i < t]
        if not ents:
            out.append(0.0)
            continue
        d = []
        for k, _ in ents:
            s = 0.0
            for c in range(H):
                s += float(vec[t, c]) * float(k[c])
            d.append(s)
        w = [math.exp(theta * (x - max(d))) for x in d]
        out.append(sum(wi for wi, (_, v) in zip(w, ents) if v == int(val[t])) / sum(w))
    return np.array(out)


@pytest.mark.parametrize('T,H,Mg,W', [(1, 3, 0, 1), (6, 4, 0, 2), (9, 5, 3, 1), (20, 7, 17, 5), (20, 7, 0, 64), (33, 6, 2, 16)])
def test_restatement_against_the_triple_loop(T, H, Mg, W):
    vec, val, keys, vals = _case(T + Mg, T, H, Mg)
    thetas = [0.0, 0.7, 3.0]
    got = SC.attend(vec, val, W, thetas, keys, vals)
    for k, th in enumerate(thetas):
        assert np.allclose(got[k], _brute(vec, val, W, th, keys, vals), rtol=1e-12, atol=0), (k, th)
    if Mg == 0:
        assert np.all(got[:, 0] == 0.0)                            # the empty set
    see = SC.visible(T, W, Mg)
    assert see.shape == (T, Mg + T) and np.array_equal(see[:, Mg:].sum(axis=1), np.minimum(np.arange(T), W))
    assert not see[:, Mg:][np.triu_indices(T)].any()                # strictly causal: no entry t or later


@pytest.mark.parametrize('Mg', [0, 5])
def test_position_equals_cache_attend_over_the_explicit_list(Mg):
    T, H = 21, 6
    vec, val, keys, vals = _case(3 + Mg, T, H, Mg)
    thetas = [0.0, 1.3]
    for W in (1, 4, 16, 17, 40):
        got = SC.attend(vec, val, W, thetas, keys, vals)
        for t in range(T):
            k, v = SC.explicit_entries(vec, val, t, W, keys, vals)
            assert len(v) == Mg + min(t, W)
            if len(v) == 0:
                assert np.all(got[:, t] == 0.0)
                continue
            want = R.attend(k, v, vec[t:t + 1], val[t:t + 1], thetas)[:, 0]
            assert np.allclose(got[:, t], want, rtol=1e-12, atol=0), (W, t)


def test_full_window_without_support_is_a_prefix_cache():
    T, H = 18, 5
    vec, val, _, _ = _case(9, T, H, 0)
    thetas = [0.5, 2.0]
    for W in (T, T + 1, 1000):
        got = SC.attend(vec, val, W, thetas)
        for t in range(1, T):
            want = R.attend(vec[:t], val[:t], vec[t:t + 1], val[t:t + 1], thetas)[:, 0]
            assert np.allclose(got[:, t], want, rtol=1e-12, atol=0), (W, t)
    rows = SC.attend_rows(np.stack([vec, vec[::-1]]), np.stack([val, val[::-1]]), T, thetas)
    assert np.array_equal(rows[:, 0], SC.attend(vec, val, T, thetas))           # a row's result does not depend on the other rows


def test_fp32_mode_is_fp32_and_close():
    vec, val, keys, vals = _case(4, 33, 200, 17)
    p64 = SC.attend(vec.astype(np.float32), val, 16, [1.0], keys.astype(np.float32), vals)
    p32 = SC.attend(vec.astype(np.float32), val, 16, [1.0], keys.astype(np.float32), vals, np.float32)
    assert p32.dtype == np.float32 and np.array_equal(p32 == 0, p64 == 0)
    pos = p64 > 0
    assert (np.abs(p32[pos] - p64[pos]) / p64[pos]).max() < 1e-3


def test_empty_set_rule():
    lp = np.log(np.array([0.5, 0.01, 0.2, 0.3], np.float32))
    pc = np.array([0.0, 0.0, 0.5, 1.0], np.float32)
    empty = SC.empty_positions(4, with_support=False)
    assert empty.tolist() == [True, False, False, False] and not SC.empty_positions(4, with_support=True).any()
    for lam in (0.0, 0.25, 1.0):
        got = SC.mix(lp, pc, lam, empty)
        assert got.dtype == np.float32 and got[0].view(np.uint32) == lp[0].view(np.uint32)      # the model alone, bitwise, lambda = 1 too
        assert np.array_equal(got[1:].view(np.uint32), R.mix(lp, pc, lam)[1:].view(np.uint32))
        assert SC.mix64(lp, pc, lam, empty)[0] == np.float64(lp[0])
    assert SC.mix(lp, pc, 1.0, empty)[1] == -np.inf                 # a non-empty set without the target: no mass at lambda = 1
    assert SC.mix(lp, pc, 1.0, np.zeros(4, bool))[0] == -np.inf     # (with support entries position 0 is an ordinary position)


@pytest.mark.parametrize('name', ['H24', 'H200x2', 'H512'])
def test_copied_half_song_gains_on_the_fp64_oracle(name):
    """The reference number of test_selfcache's copied-half leg: the per-token gain of the mixture over the model alone at lambda =
    0.25, pure self-cache, W = T.  At config/cache_lstm.yaml's theta = 1 the fp64 mixture gains 0.87 / 0.84 / 0.82 nats per token at
    H24 / H200x2 / H512, so the default is kept; gain_theta() would fall back to the best theta of tune's grid where it gave none
    (which of the two happened is printed)."""
    case = SC.oracle_case(name)
    cfg = case['cfg']
    T = cfg['max_len']
    song = case['query'][0]
    assert np.array_equal(song[T // 2:], song[:T - T // 2])
    theta, gain, kept = SC.gain_theta(case)
    print('%s: fp64 copied-half gain %.4f nats/token at theta %.3g (%s), lambda %.2f'
          % (name, gain, theta, 'the default' if kept else "picked from tune's grid: no gain at the default", SC.GAIN_LAMBDA))
    assert gain > 0
    # the second half is where the gain comes from: its targets sit in the own history with near-identical keys
    ref = SC.score(case['params'], case['query'][:1], T, [theta], [SC.GAIN_LAMBDA], cfg)
    d = ref['logprob'][0, 0, 0] - ref['lstm_logprob'][0]
    assert d[T // 2 + 1:].mean() > d[:T // 2].mean()
    assert ref['logprob'][0, 0, 0, 0] == ref['lstm_logprob'][0, 0]  # position 0: the empty set


def test_config_layout_matches_the_header():
    from fsmg import binding as B
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert C.sizeof(B.FsmgCacheSelfConfig) == 64
    assert int(re.search(r'#define FSMG_CACHE_SELF_CONFIG_VERSION (\d+)', text).group(1)) == B.FSMG_CACHE_SELF_CONFIG_VERSION
    body = re.search(r'typedef struct fsmg_cache_self_config \{(.*?)\} fsmg_cache_self_config;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;', body)
    assert [(n, int(k or 1)) for _, n, k in fields] == [(n, C.sizeof(t) // 4) for n, t in B.FsmgCacheSelfConfig._fields_]
    c = B.FsmgModel.cache_self_config(7)
    assert (c.version, c.window) == (1, 7) and not any(c.reserved)


def test_entry_points_are_declared_bound_exported_and_refuse_a_null_handle():
    from fsmg.build import build
    build()
    from fsmg import binding as B
    out = subprocess.check_output(['nm', '-D', '--defined-only', B.library_path()], universal_newlines=True)
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    for name in SELF_ENTRY_POINTS:
        assert name in B.SIGNATURES and re.search(r' T %s$' % name, out, flags=re.M) and re.search(r'\bint %s\(' % name, text), name
    assert 'k_cache_attend_self' in open(B.library_path(), 'rb').read().decode('latin-1')
    lib = B.load_library()
    cs = B.FsmgModel.cache_score_config(2, [1.0], [0.5])
    sc = B.FsmgModel.cache_self_config(4)
    toks = np.zeros((2, 4), np.int32)
    f = np.zeros(64, np.float32)
    i = np.zeros(8, np.int32)
    tp, fp, ip = C.c_void_p(toks.ctypes.data), f.ctypes.data_as(C.POINTER(C.c_float)), i.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.fsmg_cache_self_score(None, None, C.byref(cs), C.byref(sc), tp, None, fp, None, None, None) == -1
    assert lib.fsmg_cache_self_attend(None, None, C.byref(sc), 1, 2, fp, ip, None, fp, 1, fp) == -1


def test_plugin_config_and_yaml_need_no_device():
    import yaml
    from conftest import small_config
    from models.cache_lstm import CacheLSTM
    with pytest.raises(RuntimeError, match='cache_window'):
        CacheLSTM(dict(small_config(), cache_theta=1.0, cache_lambda=0.5, cache_self=True, cache_window=0))
    conf = os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config')
    cfg = yaml.safe_load(open(os.path.join(conf, 'cache_self_lstm.yaml')))
    base = yaml.safe_load(open(os.path.join(conf, 'cache_lstm.yaml')))
    assert cfg['cache_self'] is True and cfg['name'] == 'cache_self_lstm' and 'cache_self' not in base and 'cache_window' not in base
    assert {k: v for k, v in cfg.items() if k not in ('name', 'cache_self')} == {k: v for k, v in base.items() if k != 'name'}


SELF_ENTRY_POINTS = ('fsmg_cache_self_score', 'fsmg_cache_self_attend', 'fsmg_cache_self_generate', 'fsmg_cache_self_distribution')
