"""fsmg_score / fsmg_maml_score on the MI355X against the fp64 numpy restatement of their contract (tests/score_ref.py): known
answers with exact ranks, the GPU's own logits, the fp64 oracle, the existing entry points, passes, windows and NULL outputs,
side effects, MAML, NaN rows, errors and the plugin surface."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import score_ref as S
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

ALL = dict(logprob=True, rank=True, entropy=True, argmax=True, row_nll=True)
KEYS = ('logprob', 'rank', 'entropy', 'argmax', 'row_nll')
TOL = 1e-5          # log-prob / entropy against fp64 on the same fp32 logits, scaled by max(1, |value|): test_gpu_parity's lse / ce bound


def _trained(cfg, steps=3, seed=7, **kw):
    m = new_model(cfg, **kw)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


def _songs(cfg, R, seed=0):
    return np.random.RandomState(seed).randint(0, cfg['input_size'], size=(R, cfg['max_len'])).astype(np.int32)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _scaled_err(got, want):
    """max |got - want| / max(1, |want|) over the finite entries; the non-finite ones must agree exactly"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin])
    return float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max()) if fin.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. known answers
@pytest.mark.parametrize('V1', [98, 1025, 50001])
def test_known_answers_exact_ranks(V1):
    """softmax_w = 0: the logits of every position are softmax_b exactly -- gaps of 0.01, two tied pairs, one -inf column"""
    cfg = small_config(input_size=V1 - 1, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    b, cols = S.known_bias(V1)
    m.set_param('softmax_w', np.zeros((16, V1), np.float32))
    m.set_param('softmax_b', b)
    songs = S.known_songs(V1, 4, 8, cols)
    got = m.score(songs, **ALL)
    y = songs.reshape(-1)
    lp, rk, en, am = S.score_rows(np.broadcast_to(b.astype(np.float64), (y.size, V1)), y)
    assert np.array_equal(got['rank'].reshape(-1), rk)
    assert np.array_equal(got['argmax'].reshape(-1), am)
    e_lp, e_en = _scaled_err(got['logprob'].reshape(-1), lp), _scaled_err(got['entropy'].reshape(-1), en)
    print('V1 = %d: log-prob error %.3g, entropy error %.3g' % (V1, e_lp, e_en))
    assert e_lp <= TOL and e_en <= TOL
    # what the bias was built for: a tied pair ranks by index, the -inf target ranks last
    r = dict(zip(y.tolist(), got['rank'].reshape(-1).tolist()))
    for lo, hi in (cols['pair_a'], cols['pair_b']):
        assert r[hi] == r[lo] + 1
    assert r[cols['neg_inf']] == V1 - 1 and got['logprob'].reshape(-1)[list(y).index(cols['neg_inf'])] == -np.inf


# ------------------------------------------------------------------------------------------------ 2 + 3. own logits, fp64 oracle
SHAPES = {
    'H24': (dict(input_size=300, max_len=16, embedding_size=20, hidden_size=24, n_layers=1), 7),
    'H200x2': (dict(input_size=300, max_len=16, embedding_size=20, hidden_size=200, n_layers=2), 7),
    'H512': (dict(input_size=300, max_len=16, embedding_size=20, hidden_size=512, n_layers=1), 7),
    'H1024x2': (dict(input_size=300, max_len=16, embedding_size=20, hidden_size=1024, n_layers=2), 7),
    'cfg-B': (dict(input_size=10000, max_len=32, embedding_size=250, hidden_size=512, n_layers=1), 64),
}


@functools.lru_cache(maxsize=None)
def _scored(name):
    """one trained model per shape, scored once: (cfg, songs, outputs, the pass's fp32 logits time-major, fp64 parameters)"""
    over, R = SHAPES[name]
    cfg = small_config(**over)
    m = _trained(cfg, steps=2 if name == 'cfg-B' else 3)
    songs = _songs(cfg, R, seed=5)
    got = m.score(songs, **ALL)
    d = m.debug_dims()
    T, V1 = cfg['max_len'], cfg['input_size'] + 1
    logits = m.debug_read('logits', T * R * d['V1p']).reshape(T * R, d['V1p'])[:, :V1].copy()
    params = f64_params(m)
    m.close()
    return cfg, songs, got, logits, params


@pytest.mark.parametrize('name', list(SHAPES))
def test_against_the_gpus_own_logits(name):
    cfg, songs, got, logits, _ = _scored(name)
    R, T = songs.shape
    y = songs.T.reshape(-1)                                    # time-major, like the logits' rows t * R + b
    lp, rk, en, am = S.score_rows(logits, y)
    tm = lambda a: a.reshape(T, R).T
    assert np.array_equal(got['rank'], tm(rk))
    assert np.array_equal(got['argmax'], tm(am))
    e_lp, e_en = _scaled_err(got['logprob'], tm(lp)), _scaled_err(got['entropy'], tm(en))
    print('%s: log-prob error %.3g, entropy error %.3g against fp64 on the fp32 logits' % (name, e_lp, e_en))
    assert e_lp <= TOL and e_en <= TOL
    assert np.array_equal(got['row_nll'].view(np.uint32), S.row_nll(got['logprob']).view(np.uint32))


@pytest.mark.parametrize('name', list(SHAPES))
def test_against_the_fp64_oracle(name):
    cfg, songs, got, _, params = _scored(name)
    R, T = songs.shape
    z, y = S.oracle_logits(params, songs, cfg)
    lp, rk, en, am = S.score_rows(z, y)
    e_lp = np.abs(got['logprob'] - lp.reshape(R, T)).max()
    e_en = np.abs(got['entropy'] - en.reshape(R, T)).max()
    e_nll = np.abs(got['row_nll'] + lp.reshape(R, T).mean(axis=1)).max()
    print('%s: |log-prob| %.3g, |entropy| %.3g, |row_nll| %.3g against the fp64 oracle' % (name, e_lp, e_en, e_nll))
    assert e_lp <= 1e-4 and e_en <= 1e-4 and e_nll <= 1e-4
    lo, hi = S.rank_band(z, y, 4e-5)                           # twice the project's 2e-5 logit bound; every position
    rank = got['rank'].reshape(-1)
    assert np.all(lo <= rank) and np.all(rank <= hi), np.flatnonzero((rank < lo) | (rank > hi))[:10]


# ------------------------------------------------------------------------------------------------ 4. existing entry points
def test_mean_equals_eval_step_and_generate_logprobs():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=48, n_layers=2)
    m = _trained(cfg)
    qry = _songs(cfg, 6, seed=2).reshape(2, 3, 12)
    got = m.score(qry)
    assert got['logprob'].shape == (6, 12) and got['row_nll'].shape == (6,)
    assert abs(float(-got['logprob'].astype(np.float64).mean()) - m.eval_step(qry)) <= 1e-4
    # a model that never emits the start word (column input_size is no token a song can hold)
    b = m.get_param('softmax_b')
    b[97] = -np.inf
    m.set_param('softmax_b', b)
    toks, lps = m.generate(9, 12, temperature=1.0, seed=4, logprobs=True)
    assert toks.max() < 97
    err = np.abs(m.score(toks)['logprob'] - lps).max()
    print('score against generate: %.3g' % err)
    assert err <= 2e-4


# ------------------------------------------------------------------------------------------------ 5. passes
def test_passes_are_calls_of_their_own():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    m = _trained(cfg)
    songs = _songs(cfg, 300, seed=3)
    whole = m.score(songs, pass_rows=128, **ALL)
    parts = [m.score(songs[a:b], pass_rows=128, **ALL) for a, b in ((0, 128), (128, 256), (256, 300))]
    _same_bits(whole, {k: np.concatenate([p[k] for p in parts]) for k in KEYS})
    _same_bits(whole, m.score(songs, pass_rows=128, **ALL))   # the same call twice
    _same_bits(whole, m.score(songs, **ALL))                   # 0 = the header's default, 128
    one = m.score(songs[:1], **ALL)
    assert one['logprob'].shape == (1, 12) and one['row_nll'].shape == (1,)
    _same_bits(one, m.score(songs[:1], **ALL))
    r129 = m.score(songs[:129], pass_rows=128, **ALL)
    _same_bits(r129, {k: np.concatenate([parts[0][k], m.score(songs[128:129], **ALL)[k]]) for k in KEYS})
    # the pass size comes from the config, not from what the handle ran before: a handle that has grown for 300-row passes
    big = m.score(songs, pass_rows=300, **ALL)
    assert big['rank'].shape == (300, 12)
    _same_bits(whole, m.score(songs, pass_rows=128, **ALL))


def test_time_out_repeats_the_pass_on_per_step_launches():
    """chain_spin_limit 0 makes a persistent recurrent kernel give up at once (the handle's own knob for this path): the pass is
    repeated on per-step launches inside the call, as fsmg_eval_batch does, and gives a per-step handle's bits"""
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=512)
    a, b = _trained(cfg), _trained(cfg)
    songs = _songs(cfg, 20, seed=8)
    first = a.score(songs, **ALL)
    st = a.stats()
    assert st['xcd_launches'] + st['persistent_launches'] > 0 and st['timeouts'] == 0
    a.debug_set('chain_spin_limit', 0)
    got = a.score(songs, **ALL)
    st = a.stats()
    assert st['timeouts'] == 1 and not st['persistent_path']
    a.debug_set('chain_spin_limit', 1 << 18)
    b.debug_set('persistent', 0)
    _same_bits(got, b.score(songs, **ALL))
    for k in ('logprob', 'entropy'):                           # two kernel families, each within 1e-4 of fp64
        assert np.abs(got[k] - first[k]).max() <= 2e-4, k
    _same_bits(got, a.score(songs, **ALL))                     # the handle goes on (fallback period: still per step)


# ------------------------------------------------------------------------------------------------ 6. window, NULLs, device tokens
def test_window_null_outputs_and_device_tokens():
    import torch
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    m = _trained(cfg)
    songs = _songs(cfg, 10, seed=4)
    full = m.score(songs, nll_first=4, nll_count=5, **ALL)
    assert np.array_equal(full['row_nll'].view(np.uint32), S.row_nll(full['logprob'], 4, 5).view(np.uint32))
    tail = m.score(songs, nll_first=7, **ALL)                  # count 0: up to T
    assert np.array_equal(tail['row_nll'].view(np.uint32), S.row_nll(full['logprob'], 7, 0).view(np.uint32))
    for n in range(1, 6):
        for subset in itertools.combinations(KEYS, n):
            got = m.score(songs, nll_first=4, nll_count=5, **{k: k in subset for k in KEYS})
            assert set(got) == set(subset)
            _same_bits(full, got, subset)
    dev = torch.tensor(songs, dtype=torch.int32, device='cuda')
    _same_bits(full, m.score(dev.data_ptr(), n_rows=10, nll_first=4, nll_count=5, **ALL))


# ------------------------------------------------------------------------------------------------ 7. no side effects
def _state(m):
    return m.get_params(), {k: m.get_opt_state(k) for k in m.param_shapes}, m.step, m.read_losses(2)


def _same_state(a, b):
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)), k
        assert np.array_equal(a[1][k][0], b[1][k][0]) and np.array_equal(a[1][k][1], b[1][k][1]), k
    assert a[2] == b[2] and np.array_equal(a[3], b[3])


def test_no_side_effects():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    sup, qry = O.synthetic_episodes(1, 2, 2, 2, 12, 97, seed=3)[0]
    m1, m2 = _trained(cfg), _trained(cfg)
    m1.forward_backward(sup, qry)
    m2.forward_backward(sup, qry)
    before, grads = _state(m1), {k: m1.get_grad(k) for k in m1.param_shapes}
    m1.score(_songs(cfg, 9, seed=6), **ALL)
    _same_state(before, _state(m1))
    for k, g in grads.items():
        assert np.array_equal(g.view(np.uint32), m1.get_grad(k).view(np.uint32)), k
    assert m1.apply_update() == m2.apply_update()
    m1.score(_songs(cfg, 9, seed=6), **ALL)
    assert m1.train_step(sup, qry) == m2.train_step(sup, qry)
    for k, v in m1.get_params().items():
        assert np.array_equal(v, m2.get_param(k)), k


# ------------------------------------------------------------------------------------------------ 8. MAML
def test_maml_score_adapts_restores_and_matches_oracle():
    cfg = small_config(input_size=60, max_len=10, embedding_size=10, hidden_size=32)
    m = _trained(cfg)
    rng = np.random.RandomState(4)
    support = rng.randint(0, 60, size=(1, 3, 10)).astype(np.int32)
    query = rng.randint(0, 60, size=(1, 4, 10)).astype(np.int32)
    theta = m.get_params()
    plain = m.score(query, **ALL)
    got = m.maml_score(support, query, 2, 0.1, **ALL)
    for k, v in m.get_params().items():
        assert np.array_equal(v.view(np.uint32), theta[k].view(np.uint32)), k
    fast, _ = O.maml_adapt({k: v.astype(np.float64) for k, v in theta.items()}, support, cfg, inner_steps=2, inner_lr=0.1)
    want = S.score_songs(fast, query, cfg)
    for k in ('logprob', 'entropy', 'row_nll'):
        assert np.abs(got[k] - want[k]).max() <= 1e-4, k
    z, y = S.oracle_logits(fast, query, cfg)
    lo, hi = S.rank_band(z, y, 4e-5)
    assert np.all(lo <= got['rank'].reshape(-1)) and np.all(got['rank'].reshape(-1) <= hi)
    assert abs(float(-got['logprob'].astype(np.float64).mean()) - m.maml_eval(support, query, 2, 0.1)) <= 1e-4
    assert not np.array_equal(got['logprob'], plain['logprob'])
    _same_bits(plain, m.score(query, **ALL))                   # theta is back: the unadapted scores are what they were


# ------------------------------------------------------------------------------------------------ 9. NaN rows, errors
@pytest.mark.parametrize('input_size', [97, 40000])
def test_nan_logits_give_nan_scores_and_in_range_integers(input_size):
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    m.set_param('softmax_b', np.full(input_size + 1, np.nan, np.float32))
    got = m.score(_songs(cfg, 5), **ALL)
    assert np.all(np.isnan(got['logprob'])) and np.all(np.isnan(got['entropy'])) and np.all(np.isnan(got['row_nll']))
    for k in ('rank', 'argmax'):
        assert np.all((got[k] >= 0) & (got[k] <= input_size)), k
    m.set_param('softmax_b', np.zeros(input_size + 1, np.float32))
    got = m.score(_songs(cfg, 5), **ALL)                       # the handle stays usable
    assert np.all(np.isfinite(got['logprob'])) and np.all(got['entropy'] > 0)


def test_argument_errors():
    from fsmg.binding import FsmgError
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    songs = _songs(cfg, 4)
    lp = np.empty((4, 8), np.float32)
    F32P, I32P = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def call(tokens=songs, out=lp, **over):
        c = m.score_config(4)
        for k, v in over.items():
            if k == 'reserved':
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return m._lib.fsmg_score(m._h, C.byref(c), None if tokens is None else C.c_void_p(tokens.ctypes.data),
                                 None if out is None else out.ctypes.data_as(F32P), None, None, None, None)

    assert call() == 0
    for bad in (dict(version=2), dict(version=0), dict(reserved=0), dict(reserved=9), dict(n_rows=0), dict(n_rows=-3),
                dict(tokens_on_device=2), dict(tokens_on_device=-1), dict(nll_first=-1), dict(nll_first=8), dict(nll_count=-1),
                dict(nll_first=4, nll_count=5), dict(pass_rows=-1), dict(pass_rows=1025), dict(out=None), dict(tokens=None)):
        assert call(**bad) == -1, bad
    assert call(nll_first=4, nll_count=4) == 0 and call(nll_first=7) == 0 and call(pass_rows=1024) == 0 and call(pass_rows=1) == 0
    rk = np.empty((4, 8), np.int32)
    c = m.score_config(4)
    assert m._lib.fsmg_score(m._h, C.byref(c), C.c_void_p(songs.ctypes.data), None, rk.ctypes.data_as(I32P), None, None, None) == 0
    bad = songs.copy()
    bad[2, 3] = 50
    with pytest.raises(FsmgError) as e:
        m.score(bad)
    assert e.value.code == -7
    import torch
    dev = torch.tensor(bad, dtype=torch.int32, device='cuda')
    with pytest.raises(FsmgError) as e:
        m.score(dev.data_ptr(), n_rows=4)
    assert e.value.code == -7
    bad[2, 3] = -1
    with pytest.raises(FsmgError) as e:
        m.score(bad)
    assert e.value.code == -7
    with pytest.raises(FsmgError) as e:                         # the MAML variant refuses the same configs before it adapts
        m.maml_score(songs[:2], songs, 1, 0.1, nll_first=8)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        m.score(np.zeros((3, 7), np.int32))
    assert np.all(np.isfinite(m.score(songs)['logprob']))      # the handle stays usable


# ------------------------------------------------------------------------------------------------ 10. plugins
def test_plugin_score(tmp_path):
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    rng = np.random.RandomState(5)
    support = rng.randint(0, 40, size=(3, 12)).astype(np.int32)
    songs = rng.randint(0, 40, size=(5, 12)).astype(np.int32)
    for cls in (LSTMBaseline, MAMLLSTM):
        cfg = dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name=cls.__name__.lower(),
                   checkpt_dir=str(tmp_path / cls.__name__), inner_steps=1, inner_lr=0.1)
        model = cls(cfg)
        model.recover_or_init('')
        got = model.score(support, songs, **ALL)
        assert got['logprob'].shape == (5, 12) and got['rank'].dtype == np.int32 and got['row_nll'].shape == (5,)
        if cls is LSTMBaseline:
            _same_bits(got, model.engine.score(songs, **ALL))
            assert set(model.score(support, songs)) == {'logprob', 'row_nll'}
        else:
            _same_bits(got, model.engine.maml_score(support, songs, 1, 0.1, **ALL))
            assert not np.array_equal(got['logprob'], LSTMBaseline.score(model, support, songs)['logprob'])
