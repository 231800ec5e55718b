"""fsmg_generate_filtered / fsmg_maml_generate_filtered on the MI355X against the fp64 numpy restatement (tests/filter_ref.py):
neutral filters bitwise equal to fsmg_generate, teacher-forced margins, exact top-p / min-p sets and their distribution, the
repetition penalty, determinism and row independence, non-finite logits, no side effects, errors, and the plugin / train.train
surface."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_ref as F
import gen_ref as R
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

LN2 = float(np.log(2.0))


def _trained(cfg, steps=3, seed=7):
    m = new_model(cfg)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


def _filtered_raw(m, filters, B, num, T=1.0, k=0, seed=0, primer=None):
    """fsmg_generate_filtered with an explicit filters struct (or None for NULL) -> (rc, tokens, log-probs)"""
    from fsmg.binding import _I32P, _f32p
    g, pp, _keep = m._gen_args(B, num, T, k, seed, primer)
    toks = np.zeros((B, num), np.int32)
    lp = np.zeros((B, num), np.float32)
    rc = m._lib.fsmg_generate_filtered(m._h, C.byref(g), None if filters is None else C.byref(filters), pp,
                                       toks.ctypes.data_as(_I32P), _f32p(lp))
    return rc, toks, lp


def _filters(**kw):
    from fsmg.binding import FsmgGenFilters, FSMG_GEN_FILTERS_VERSION
    f = FsmgGenFilters(version=FSMG_GEN_FILTERS_VERSION)
    for k, v in kw.items():
        if k == 'reserved':
            f.reserved[v] = 1
        else:
            setattr(f, k, v)
    return f


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# -------------------------------------------------------------------------------- 1. neutral filters
@pytest.mark.parametrize('input_size', [97, 20000, 50000])
def test_neutral_filters_are_fsmg_generate_bitwise(input_size):
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
    m = _trained(cfg, steps=1)
    primer = np.random.RandomState(2).randint(0, input_size, size=(5, 3))
    neutral = [None, _filters(), _filters(repetition_penalty=1.0), _filters(top_p=1.0),
               _filters(top_p=1.0, repetition_penalty=1.0, repeat_window=5)]
    for T, k, pr in ((1.0, 0, None), (0.7, 5, primer), (0.0, 0, primer), (2.0, 1, None)):
        want, wlp = m.generate(5, 6, temperature=T, top_k=k, seed=3, primer=pr, logprobs=True)
        for f in neutral:
            rc, toks, lp = _filtered_raw(m, f, 5, 6, T, k, 3, pr)
            assert rc == 0
            assert np.array_equal(toks, want) and np.array_equal(_bits(lp), _bits(wlp)), (T, k, f)
        toks, lp = m.generate(5, 6, temperature=T, top_k=k, seed=3, primer=pr, logprobs=True, top_p=1.0, repetition_penalty=1.0)
        assert np.array_equal(toks, want) and np.array_equal(_bits(lp), _bits(wlp))


# -------------------------------------------------------------------------------- 2. teacher-forced margins
FILTER_CASES = {
    'top_p': dict(top_p=0.9),
    'min_p': dict(min_p=0.05),
    'penalty': dict(repetition_penalty=1.3, repeat_window=4),
    'all': dict(top_p=0.8, min_p=0.02, repetition_penalty=1.5, repeat_window=0),
}


def _check(m, cfg, B, num, T, k, seed, fk, primer=None, rows=None, params=None):
    toks, lps = m.generate(B, num, temperature=T, top_k=k, seed=seed, primer=primer, logprobs=True, **fk)
    assert toks.shape == (B, num) and lps.shape == (B, num)
    near = F.check_margins(f64_params(m) if params is None else params, cfg, toks, lps, T, k, seed, top_p=fk.get('top_p', 0.0),
                           min_p=fk.get('min_p', 0.0), theta=fk.get('repetition_penalty', 1.0), window=fk.get('repeat_window', 0),
                           primer=primer, rows=rows)
    return toks, lps, near


@pytest.mark.parametrize('H,L', [(24, 1), (200, 2), (512, 1), (1024, 2)])
def test_margins_across_hidden_sizes(H, L):
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)
    m = _trained(cfg)
    primer = np.random.RandomState(1).randint(0, 300, size=(5, 6))
    for name, fk in FILTER_CASES.items():
        _, _, near = _check(m, cfg, 5, 10, 1.0, 0, 11, fk)
        assert near <= 3, name
        _check(m, cfg, 5, 8, 0.7, 20, 12, fk, primer=primer)


@pytest.mark.parametrize('which', ['cfg-B', 'cfg-C'])
def test_margins_full_size(which):
    if which == 'cfg-B':
        cfg = small_config(input_size=10000, max_len=32, embedding_size=250, hidden_size=512, n_layers=1)
    else:
        cfg = small_config(input_size=4708, max_len=32, embedding_size=250, hidden_size=1024, n_layers=2)
    m = _trained(cfg, steps=2)
    _check(m, cfg, 64, 24, 1.0, 0, 5, FILTER_CASES['all'], rows=range(0, 64, 13))
    _check(m, cfg, 16, 16, 1.0, 0, 6, dict(top_p=0.5), rows=range(0, 16, 5))


@pytest.mark.parametrize('B,P,k,T', [(7, 0, 0, 0.0), (7, 3, 5, 0.7), (16, 9, 0, 1.0), (16, 1, 1, 1.0), (9, 2, 0, 2.0), (7, 4, 'V1', 1.0)])
def test_margins_batch_primer_topk_temperature(B, P, k, T):
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32, n_layers=2)
    m = _trained(cfg)
    k = cfg['input_size'] + 1 if k == 'V1' else k
    primer = np.random.RandomState(B).randint(0, 97, size=(B, P)) if P else None
    for fk in FILTER_CASES.values():
        _check(m, cfg, B, 10, T, k, 3, fk, primer=primer, rows=range(0, B, max(1, B // 6)))


@pytest.mark.parametrize('input_size', [50000, 20000])
def test_margins_vocabulary_larger_than_lds(input_size):
    # 50 001 columns: read from global memory, the penalty as a presence bitmap in LDS; 20 001: staged above 64 KiB
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
    m = _trained(cfg, steps=1)
    primer = np.random.RandomState(3).randint(0, input_size, size=(3, 4))
    for fk in FILTER_CASES.values():
        _check(m, cfg, 3, 6, 1.0, 0, 9, fk, primer=primer)
    _check(m, cfg, 3, 6, 0.5, 40, 9, FILTER_CASES['all'])


# -------------------------------------------------------------------------------- 3. exact sets on crafted logits
def _bias_model(b):
    """every parameter 0 except softmax_b: h stays 0, so every position's logits are the bias exactly"""
    cfg = small_config(input_size=len(b) - 1, max_len=8, embedding_size=4, hidden_size=16)
    m = new_model(cfg)
    params = {k: np.zeros_like(v) for k, v in m.get_params().items()}
    params['softmax_b'] = np.asarray(b, np.float32)
    m.set_params(params)
    return m


CHI2_DF3 = 16.266       # chi-square critical value at p = 0.001, df = 3


def test_exact_sets_and_distribution():
    # q ~ .493, .247, .123, .123 and a tail of 1.4 %; top-p mass-ahead 0, .493, .740 (a tie), .986, ...
    b = np.array([0.0, -LN2, -2 * LN2, -2 * LN2, -4.0, -5.0, -6.0, -7.0], np.float32)
    m = _bias_model(b)
    cases = [(dict(top_p=0.3), 1.0, 0, [0]), (dict(top_p=0.6), 1.0, 0, [0, 1]), (dict(top_p=0.8), 1.0, 0, [0, 1, 2, 3]),
             (dict(min_p=0.3), 1.0, 0, [0, 1]), (dict(min_p=0.2), 1.0, 0, [0, 1, 2, 3]), (dict(min_p=0.45), 2.0, 0, [0, 1, 2, 3]),
             (dict(min_p=0.9), 1.0, 0, [0]), (dict(top_p=0.99), 1.0, 2, [0, 1]), (dict(top_p=0.9, min_p=0.01), 0.5, 0, [0, 1])]
    for fk, T, k, want in cases:
        toks = m.generate(512, 32, temperature=T, top_k=k, seed=5, **fk)
        assert sorted(np.unique(toks).tolist()) == want, (fk, T, k, np.unique(toks))
    for fk, seed in ((dict(top_p=0.8), 1), (dict(min_p=0.2), 2)):
        toks = m.generate(1024, 64, temperature=1.0, seed=seed, **fk)
        counts = np.bincount(toks.ravel(), minlength=8)[:4].astype(np.float64)
        p = np.exp(b[:4].astype(np.float64) - R.logsumexp(b[:4].astype(np.float64)))
        chi2 = np.sum((counts - p * toks.size) ** 2 / (p * toks.size))
        assert counts.sum() == toks.size and chi2 < CHI2_DF3, (fk, chi2, counts, p * toks.size)


# -------------------------------------------------------------------------------- 4. the penalty, exactly
@pytest.mark.parametrize('input_size', [40, 40000])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_penalty_cycles_greedy_through_the_window(input_size, sign):
    V1 = input_size + 1
    b = (sign * (2.0 + 0.5 * np.arange(V1)[::-1] / V1)).astype(np.float32)
    if sign < 0:
        b = (-2.0 - 0.5 * np.arange(V1) / V1).astype(np.float32)   # all negative, column 0 best: the multiply branch
    m = _bias_model(b)
    assert m.generate(1, 6, temperature=0.0).tolist() == [[0] * 6]
    for n in (1, 3, 7):
        toks = m.generate(2, 20, temperature=0.0, repetition_penalty=1e6, repeat_window=n)
        assert toks.tolist() == [[t % (n + 1) for t in range(20)]] * 2, (n, toks)
    toks = m.generate(1, 12, temperature=0.0, repetition_penalty=1e6)          # the whole context
    assert toks.tolist() == [list(range(12))]
    # the primer's ids start out penalised; the start word is not part of the context
    toks = m.generate(1, 6, temperature=0.0, repetition_penalty=1e6, primer=np.array([[0, 2]]))
    assert toks.tolist() == [[1, 3, 4, 5, 6, 7]]
    toks = m.generate(1, 4, temperature=0.0, repetition_penalty=1e6, repeat_window=1, primer=np.array([[0, 2]]))
    assert toks.tolist() == [[0, 1, 0, 1]]
    # with sampling on, a huge penalty still keeps every draw out of the window
    toks = m.generate(4, 16, temperature=1.0, seed=3, repetition_penalty=1e6, repeat_window=3, top_p=0.5)
    for row in toks.tolist():
        for t in range(16):
            assert row[t] not in row[max(0, t - 3):t], row


# -------------------------------------------------------------------------------- 5. determinism and row independence
def test_determinism_and_row_independence():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=64, n_layers=2)
    m = _trained(cfg)
    primer = np.random.RandomState(0).randint(0, 97, size=(300, 4))
    fk = dict(top_p=0.85, min_p=0.03, repetition_penalty=1.4, repeat_window=6)
    a, la = m.generate(16, 20, temperature=1.0, top_k=30, seed=42, primer=primer[:16], logprobs=True, **fk)
    b, lb = m.generate(16, 20, temperature=1.0, top_k=30, seed=42, primer=primer[:16], logprobs=True, **fk)
    assert np.array_equal(a, b) and np.array_equal(_bits(la), _bits(lb))
    c = m.generate(16, 20, temperature=1.0, top_k=30, seed=43, primer=primer[:16], **fk)
    assert not np.array_equal(a, c)
    d, ld = m.generate(300, 20, temperature=1.0, top_k=30, seed=42, primer=primer, logprobs=True, **fk)
    assert np.array_equal(a, d[:16]) and np.array_equal(_bits(la), _bits(ld[:16]))


# -------------------------------------------------------------------------------- 6. non-finite logits
@pytest.mark.parametrize('input_size', [97, 40000])
def test_non_finite_logits(input_size):
    V1 = input_size + 1
    rs = np.random.RandomState(1)
    fks = [dict(top_p=0.9), dict(min_p=0.1), dict(repetition_penalty=1.5, repeat_window=3), FILTER_CASES['all']]
    for kind in ('nan', 'half_nan', 'inf', 'neg_inf'):
        b = rs.randn(V1).astype(np.float32)
        if kind == 'nan':
            b[:] = np.nan
        elif kind == 'half_nan':
            b[::2] = np.nan
        elif kind == 'inf':
            b[[3, 7]] = np.inf
            b[::5] = np.nan
        else:
            b[:] = -np.inf
            b[::3] = np.nan
        m = _bias_model(b)
        for fk in fks:
            for T, k in ((1.0, 0), (0.7, 3), (0.0, 0)):
                toks = m.generate(4, 5, temperature=T, top_k=k, seed=2, primer=np.full((4, 2), 3, np.int32), **fk)
                assert np.all((toks >= 0) & (toks < V1)), (kind, fk, T, k, toks)
                if kind != 'nan':               # a NaN column is never drawn while a comparable one exists
                    assert not np.any(np.isnan(b[toks])), (kind, fk, T, k, toks)
                if kind == 'inf' and 'repetition_penalty' not in fk:
                    assert set(np.unique(toks).tolist()) <= {3, 7}, (fk, T, k, toks)
        m.close()


# -------------------------------------------------------------------------------- 7. state
def _state(m):
    opt = {k: m.get_opt_state(k) for k in m.param_shapes}
    return m.get_params(), opt, m.step, m.read_losses(2), m.stats()


def _same_state(a, b, skip=()):
    pa, oa, sa, la, ta = a
    pb, ob, sb, lb, tb = b
    for k in pa:
        assert np.array_equal(_bits(pa[k]), _bits(pb[k])), k
        assert np.array_equal(oa[k][0], ob[k][0]) and np.array_equal(oa[k][1], ob[k][1]), k
    assert sa == sb and np.array_equal(la, lb)
    assert {k: v for k, v in ta.items() if k not in skip} == {k: v for k, v in tb.items() if k not in skip}


def test_no_side_effects():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    sup, qry = O.synthetic_episodes(1, 2, 2, 2, 12, 97, seed=3)[0]
    m1, m2 = _trained(cfg), _trained(cfg)
    before = _state(m1)
    m1.generate(9, 15, temperature=1.0, top_k=4, seed=5, primer=np.ones((9, 2), np.int32), **FILTER_CASES['all'])
    _same_state(before, _state(m1))
    l1, l2 = m1.train_step(sup, qry), m2.train_step(sup, qry)
    assert l1 == l2


def test_maml_generate_filtered_adapts_restores_and_matches_oracle():
    cfg = small_config(input_size=60, max_len=10, embedding_size=10, hidden_size=32)
    m = _trained(cfg)
    support = np.random.RandomState(4).randint(0, 60, size=(3, 10)).astype(np.int32)
    theta = m.get_params()
    fk = FILTER_CASES['all']
    g0 = m.generate(5, 12, temperature=1.0, seed=8, **fk)
    params, opt, step, losses, stats = _state(m)
    toks, lps = m.maml_generate(support, 12, 2, 0.1, n_seq=5, temperature=1.0, seed=8, logprobs=True, **fk)
    launch_counters = ('xcd_launches', 'persistent_launches', 'step_launches')
    _same_state((params, opt, step, losses, stats), _state(m), skip=launch_counters)
    for k, v in m.get_params().items():
        assert np.array_equal(_bits(v), _bits(theta[k])), k
    fast, _ = O.maml_adapt({k: v.astype(np.float64) for k, v in theta.items()}, support[None], cfg, inner_steps=2, inner_lr=0.1)
    F.check_margins(fast, cfg, toks, lps, 1.0, 0, 8, top_p=fk['top_p'], min_p=fk['min_p'], theta=fk['repetition_penalty'],
                    window=fk['repeat_window'])
    assert np.array_equal(m.generate(5, 12, temperature=1.0, seed=8, **fk), g0)
    # neutral filters through the MAML entry point: fsmg_maml_generate's output
    a = m.maml_generate(support, 8, 2, 0.1, n_seq=3, temperature=1.0, seed=8)
    from fsmg.binding import _I32P
    g, pp, _keep = m._gen_args(3, 8, 1.0, 0, 8, None)
    out = np.zeros((3, 8), np.int32)
    rc = m._lib.fsmg_maml_generate_filtered(m._h, C.byref(g), C.byref(_filters(top_p=1.0)), C.c_void_p(support.ctypes.data), 3, 2,
                                            0.1, 0, pp, out.ctypes.data_as(_I32P), None)
    assert rc == 0 and np.array_equal(out, a)


# -------------------------------------------------------------------------------- 8. errors
def test_argument_errors():
    from fsmg.binding import FsmgError
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    assert _filtered_raw(m, _filters(top_p=0.5), 4, 4)[0] == 0
    nan, inf = float('nan'), float('inf')
    for bad in (dict(version=2), dict(version=0), dict(reserved=0), dict(reserved=7), dict(top_p=-0.1), dict(top_p=1.5),
                dict(top_p=nan), dict(min_p=-0.01), dict(min_p=1.01), dict(min_p=nan), dict(repetition_penalty=-1.0),
                dict(repetition_penalty=inf), dict(repetition_penalty=nan), dict(repeat_window=-1)):
        assert _filtered_raw(m, _filters(**bad), 4, 4)[0] == -1, bad
    g, pp, _keep = m._gen_args(4, 4, 1.0, 0, 0, None)
    g.version = 2
    assert m._lib.fsmg_generate_filtered(m._h, C.byref(g), C.byref(_filters(top_p=0.5)), None, None, None) == -1
    assert _filtered_raw(m, _filters(top_p=0.5), 4, 4, T=-1.0)[0] == -1
    assert _filtered_raw(m, _filters(top_p=0.5), 4, 4, k=52)[0] == -1
    assert _filtered_raw(m, _filters(min_p=1.0, repetition_penalty=0.0), 4, 4)[0] == 0
    rc = _filtered_raw(m, _filters(top_p=0.5), 2, 4, primer=np.array([[1, 50], [0, 0]]))[0]
    assert rc == -7
    with pytest.raises(FsmgError) as e:
        m.generate(2, 4, primer=np.array([[1, 2], [-1, 0]]), top_p=0.5)
    assert e.value.code == -7
    with pytest.raises(FsmgError) as e:
        m.maml_generate(np.ones((2, 8), np.int32), 4, 1, 0.1, n_seq=2, primer=np.array([[1, 2], [3, 51]]), min_p=0.1)
    assert e.value.code == -7
    with pytest.raises(FsmgError) as e:
        m.maml_generate(np.ones((2, 8), np.int32), 4, 1, 0.1, n_seq=2, top_p=2.0)
    assert e.value.code == -1
    assert m.generate(2, 4, seed=1, top_p=0.5).shape == (2, 4)          # the handle stays usable


# -------------------------------------------------------------------------------- 9. surface
def _plugin_cfg(tmp, name='lstm_baseline'):
    return dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name=name,
                checkpt_dir=str(tmp), inner_steps=1, inner_lr=0.1)


def test_plugin_generate_with_filters(tmp_path):
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    support = np.random.RandomState(5).randint(0, 40, size=(3, 12)).astype(np.int32)
    fk = dict(top_p=0.9, min_p=0.05, repetition_penalty=1.2, repeat_window=4)
    for cls in (LSTMBaseline, MAMLLSTM):
        model = cls(_plugin_cfg(tmp_path / cls.__name__, cls.__name__.lower()))
        model.recover_or_init('')
        a = model.generate(support, 10, n=5, temperature=1.0, top_k=5, seed=3, primer_len=4, **fk)
        assert a.shape == (5, 10) and a.dtype == np.int32 and np.all((a >= 0) & (a <= 40))
        assert np.array_equal(a, model.generate(support, 10, n=5, temperature=1.0, top_k=5, seed=3, primer_len=4, **fk))
        if cls is LSTMBaseline:
            g = model.engine.generate(5, 10, temperature=1.0, top_k=5, seed=3, primer=support[np.arange(5) % 3, :4], **fk)
            assert np.array_equal(a, g)
            greedy = model.generate(support, 8, n=2, temperature=0.0, repetition_penalty=1e6, repeat_window=2)
            for row in greedy.tolist():
                assert all(row[t] not in row[max(0, t - 2):t] for t in range(8)), row


def test_train_entry_with_filter_keys(tmp_path, golden_dir):
    import test_train_entry as E
    import train.train as T
    cfg = dict(E.LOOP, name='lstm_baseline', model_module_name='models.lstm_baseline', model_class_name='LSTMBaseline',
               seed=1, embedding_size=8, hidden_size=16, n_layers=1, lr=1e-3, max_grad_norm=5, n_decay=1000,
               sample_temperature=1.0, sample_top_k=10, sample_seed=4, sample_primer_len=3, samples_per_episode=3,
               sample_top_p=0.9, sample_min_p=0.02, sample_repetition_penalty=1.3, sample_repeat_window=8)
    p = E._write_configs(tmp_path, golden_dir, cfg)
    ck = str(tmp_path / 'ck')
    T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
    for i in range(cfg['n_samples']):
        files = sorted(os.listdir(os.path.join(ck, 'samples', 'sample_%d' % i)))
        assert files == ['model_sample_%d.txt' % j for j in range(3)] + ['support_%d.txt' % j for j in range(E.K)]
