"""fsmg_generate / fsmg_maml_generate on the MI355X against the fp64 numpy restatement (tests/gen_ref.py): teacher-forced
margins, greedy parity with fsmg_sample, determinism, row independence, the sampling distribution, no side effects, errors,
and the plugin / train.train surface."""
import os

import numpy as np
import pytest

import gen_ref as R
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu


def _trained(cfg, steps=3, seed=7, **kw):
    m = new_model(cfg, **kw)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


def _check(m, cfg, B, num, T, k, seed, primer=None, rows=None):
    toks, lps = m.generate(B, num, temperature=T, top_k=k, seed=seed, primer=primer, logprobs=True)
    assert toks.shape == (B, num) and lps.shape == (B, num)
    near = R.check_margins(f64_params(m), cfg, toks, lps, T, k, seed, primer=primer, rows=rows)
    return toks, lps, near


@pytest.mark.parametrize('H,L', [(24, 1), (200, 2), (512, 1), (1024, 2)])
def test_margins_across_hidden_sizes(H, L):
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)
    m = _trained(cfg)
    _, _, near = _check(m, cfg, 7, 12, 1.0, 0, 11)
    assert near <= 2
    primer = np.random.RandomState(1).randint(0, 300, size=(7, 9))
    _check(m, cfg, 7, 8, 0.7, 5, 12, primer=primer)


@pytest.mark.parametrize('which', ['cfg-B', 'cfg-C'])
def test_margins_full_size(which):
    if which == 'cfg-B':
        cfg = small_config(input_size=10000, max_len=32, embedding_size=250, hidden_size=512, n_layers=1)
    else:
        cfg = small_config(input_size=4708, max_len=32, embedding_size=250, hidden_size=1024, n_layers=2)
    m = _trained(cfg, steps=2)
    _check(m, cfg, 64, 32, 1.0, 0, 5, rows=range(0, 64, 9))


@pytest.mark.parametrize('B,P,k,T', [(1, 0, 0, 1.0), (7, 1, 1, 1.0), (16, 9, 5, 0.7), (300, 1, 0, 2.0), (16, 0, 'V1', 1.0),
                                     (7, 9, 0, 0.0), (16, 1, 5, 2.0)])
def test_margins_batch_primer_topk_temperature(B, P, k, T):
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32, n_layers=2)
    m = _trained(cfg)
    k = cfg['input_size'] + 1 if k == 'V1' else k
    primer = np.random.RandomState(B).randint(0, 97, size=(B, P)) if P else None
    _check(m, cfg, B, 10, T, k, 3, primer=primer, rows=range(0, B, max(1, B // 20)))


def test_margins_vocabulary_larger_than_lds():
    cfg = small_config(input_size=50000, max_len=8, embedding_size=8, hidden_size=16)
    m = _trained(cfg, steps=1)
    _check(m, cfg, 3, 6, 1.0, 0, 9)
    _check(m, cfg, 3, 6, 0.5, 40, 9)


def test_margins_row_staged_above_64_kib():
    # V1 = 20 001: the pick stages 78 KiB of the row in LDS (the raised dynamic-LDS limit)
    cfg = small_config(input_size=20000, max_len=8, embedding_size=8, hidden_size=16)
    m = _trained(cfg, steps=1)
    _check(m, cfg, 5, 6, 1.0, 0, 13)
    _check(m, cfg, 5, 6, 0.8, 25, 13)


@pytest.mark.parametrize('input_size', [97, 40000])
def test_non_finite_logits_give_in_range_tokens(input_size):
    # NaN logits (a diverged or corrupted checkpoint) compare false everywhere: every draw still names a column in [0, V1), and the
    # next position gathers that embedding row (staged rows, and rows read from global memory past 128 KiB)
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    m.set_param('softmax_b', np.full(input_size + 1, np.nan, np.float32))
    for T, k in ((1.0, 0), (0.7, 3), (0.0, 0), (1.0, 1)):
        toks = m.generate(6, 5, temperature=T, top_k=k, seed=2, primer=np.full((6, 2), 3, np.int32))
        assert np.all((toks >= 0) & (toks <= input_size)), (T, k, toks)
    m.set_param('softmax_b', np.zeros(input_size + 1, np.float32))
    toks = m.generate(3, 4, temperature=0.0)                 # the handle stays usable
    assert np.all((toks >= 0) & (toks <= input_size))


def test_greedy_rows_equal_fsmg_sample():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=48, n_layers=2)
    m = _trained(cfg)
    want = m.sample(24)
    toks, lps = m.generate(5, 24, temperature=0.0, logprobs=True)
    for b in range(5):
        assert list(toks[b]) == want
    # fsmg_sample is the driver's one-row greedy case: the greedy rows also stand against the fp64 decoder
    R.check_margins(f64_params(m), cfg, toks, lps, temperature=0.0, top_k=0, seed=0)


def test_determinism_and_row_independence():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=64, n_layers=2)
    m = _trained(cfg)
    primer = np.random.RandomState(0).randint(0, 97, size=(300, 4))
    a, la = m.generate(16, 20, temperature=1.0, top_k=7, seed=42, primer=primer[:16], logprobs=True)
    b, lb = m.generate(16, 20, temperature=1.0, top_k=7, seed=42, primer=primer[:16], logprobs=True)
    assert np.array_equal(a, b) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    c = m.generate(16, 20, temperature=1.0, top_k=7, seed=43, primer=primer[:16])
    assert not np.array_equal(a, c)
    d, ld = m.generate(300, 20, temperature=1.0, top_k=7, seed=42, primer=primer, logprobs=True)
    assert np.array_equal(a, d[:16]) and np.array_equal(la.view(np.uint32), ld[:16].view(np.uint32))


# chi-square critical values at p = 0.001 (8 categories: df = 7; the top 3: df = 2)
CHI2_DF7, CHI2_DF2 = 24.322, 13.816


def test_distribution_matches_softmax():
    cfg = small_config(input_size=7, max_len=8, embedding_size=4, hidden_size=16)
    m = new_model(cfg)
    params = {k: np.zeros_like(v) for k, v in m.get_params().items()}
    b = np.array([0.3, -0.2, 1.0, 0.0, -1.0, 0.5, 0.1, -0.4], np.float32)
    params['softmax_b'] = b
    m.set_params(params)
    for T, seed in ((1.0, 1), (0.5, 2)):
        toks = m.generate(1024, 64, temperature=T, seed=seed)
        counts = np.bincount(toks.ravel(), minlength=8).astype(np.float64)
        exp = np.exp(b / T - R.logsumexp(b / T)) * toks.size
        chi2 = np.sum((counts - exp) ** 2 / exp)
        assert chi2 < CHI2_DF7, (T, chi2, counts, exp)
    toks = m.generate(1024, 64, temperature=1.0, top_k=3, seed=3)
    top3 = np.argsort(-b)[:3]
    assert set(np.unique(toks)) <= set(top3.tolist())
    counts = np.bincount(toks.ravel(), minlength=8)[top3].astype(np.float64)
    p = np.exp(b[top3] - R.logsumexp(b[top3]))
    chi2 = np.sum((counts - p * toks.size) ** 2 / (p * toks.size))
    assert chi2 < CHI2_DF2, chi2


def _state(m):
    opt = {k: m.get_opt_state(k) for k in m.param_shapes}
    stats = m.stats()
    return m.get_params(), opt, m.step, m.read_losses(2), stats


def _same_state(a, b):
    pa, oa, sa, la, ta = a
    pb, ob, sb, lb, tb = b
    for k in pa:
        assert np.array_equal(pa[k].view(np.uint32), pb[k].view(np.uint32)), k
        assert np.array_equal(oa[k][0], ob[k][0]) and np.array_equal(oa[k][1], ob[k][1]), k
    assert sa == sb and np.array_equal(la, lb) and ta == tb


def test_no_side_effects():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    sup, qry = O.synthetic_episodes(1, 2, 2, 2, 12, 97, seed=3)[0]
    m1, m2 = _trained(cfg), _trained(cfg)
    before = _state(m1)
    m1.generate(9, 15, temperature=1.0, top_k=4, seed=5, primer=np.ones((9, 2), np.int32))
    _same_state(before, _state(m1))
    l1, l2 = m1.train_step(sup, qry), m2.train_step(sup, qry)
    assert l1 == l2
    for k, v in m1.get_params().items():
        assert np.array_equal(v, m2.get_param(k)), k


def test_maml_generate_adapts_restores_and_matches_oracle():
    cfg = small_config(input_size=60, max_len=10, embedding_size=10, hidden_size=32)
    m = _trained(cfg)
    support = np.random.RandomState(4).randint(0, 60, size=(3, 10)).astype(np.int32)
    theta = m.get_params()
    g0 = m.generate(5, 12, temperature=1.0, seed=8)
    toks, lps = m.maml_generate(support, 12, 2, 0.1, n_seq=5, temperature=1.0, seed=8, logprobs=True)
    for k, v in m.get_params().items():
        assert np.array_equal(v.view(np.uint32), theta[k].view(np.uint32)), k
    fast, _ = O.maml_adapt({k: v.astype(np.float64) for k, v in theta.items()}, support[None], cfg, inner_steps=2, inner_lr=0.1)
    R.check_margins(fast, cfg, toks, lps, 1.0, 0, 8)
    assert np.array_equal(m.generate(5, 12, temperature=1.0, seed=8), g0)


def test_maml_generate_state_changes_are_the_documented_ones():
    # include/fsmg.h: like fsmg_maml_eval, only the gradient buffer and the recurrent-launch counters of the statistics move
    cfg = small_config(input_size=60, max_len=10, embedding_size=10, hidden_size=32)
    m = _trained(cfg)
    support = np.random.RandomState(6).randint(0, 60, size=(4, 10)).astype(np.int32)
    params, opt, step, losses, stats = _state(m)
    m.maml_generate(support, 8, 2, 0.1, n_seq=3, temperature=1.0, seed=1)
    params2, opt2, step2, losses2, stats2 = _state(m)
    launch_counters = ('xcd_launches', 'persistent_launches', 'step_launches')
    _same_state((params, opt, step, losses, {k: v for k, v in stats.items() if k not in launch_counters}),
                (params2, opt2, step2, losses2, {k: v for k, v in stats2.items() if k not in launch_counters}))
    assert all(stats2[k] >= stats[k] for k in launch_counters)


def test_argument_errors():
    from fsmg.binding import FsmgError
    import ctypes as C
    cfg = small_config(input_size=50, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    out = np.empty((4, 4), np.int32)

    def call(**over):
        g = m.gen_config(4, 4, 1.0, 0, 0)
        for k, v in over.items():
            if k == 'reserved':
                g.reserved[v] = 1
            else:
                setattr(g, k, v)
        return m._lib.fsmg_generate(m._h, C.byref(g), None, out.ctypes.data_as(C.POINTER(C.c_int32)), None)

    assert call() == 0
    for bad in (dict(version=2), dict(n_seq=0), dict(n_seq=-1), dict(num=-1), dict(temperature=-0.5),
                dict(temperature=float('nan')), dict(temperature=float('inf')), dict(top_k=-1), dict(top_k=52),
                dict(reserved=0), dict(reserved=6)):
        assert call(**bad) == -1, bad
    assert call(top_k=51) == 0
    with pytest.raises(FsmgError) as e:
        m.generate(2, 4, primer=np.array([[1, 50], [0, 0]]))
    assert e.value.code == -7
    import torch
    dp = torch.tensor([[1, 2], [3, -1]], dtype=torch.int32, device='cuda')
    with pytest.raises(FsmgError) as e:
        m.generate(2, 4, primer=(dp.data_ptr(), 2))
    assert e.value.code == -7
    dp[1, 1] = 4
    host = m.generate(2, 4, primer=np.array([[1, 2], [3, 4]]), seed=3)
    assert np.array_equal(m.generate(2, 4, primer=(dp.data_ptr(), 2), seed=3), host)


def _plugin_cfg(tmp, name='lstm_baseline'):
    return dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name=name,
                checkpt_dir=str(tmp), inner_steps=1, inner_lr=0.1)


def test_plugin_generate(tmp_path):
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    support = np.random.RandomState(5).randint(0, 40, size=(3, 12)).astype(np.int32)
    for cls in (LSTMBaseline, MAMLLSTM):
        model = cls(_plugin_cfg(tmp_path / cls.__name__, cls.__name__.lower()))
        model.recover_or_init('')
        a = model.generate(support, 10, n=5, temperature=1.0, top_k=5, seed=3, primer_len=4)
        assert a.shape == (5, 10) and a.dtype == np.int32
        assert np.array_equal(a, model.generate(support, 10, n=5, temperature=1.0, top_k=5, seed=3, primer_len=4))
        assert np.all((a >= 0) & (a <= 40))
        if cls is LSTMBaseline:
            # the primer is the support songs' first tokens, dealt round-robin; greedy rows are fsmg_sample's
            g = model.engine.generate(5, 10, temperature=1.0, top_k=5, seed=3, primer=support[np.arange(5) % 3, :4])
            assert np.array_equal(a, g)
            assert model.generate(support, 6, n=2, temperature=0.0).tolist() == [model.sample(support, 6)] * 2
        else:
            # drawn at theta' adapted on the support set: the model log-probabilities differ from the unadapted draw's
            _, lp = model.generate(support, 10, n=5, temperature=1.0, seed=3, logprobs=True)
            _, lp0 = LSTMBaseline.generate(model, support, 10, n=5, temperature=1.0, seed=3, logprobs=True)
            assert not np.array_equal(lp, lp0)


def test_train_entry_with_and_without_generation_keys(tmp_path, golden_dir):
    import test_train_entry as E
    import train.train as T
    for with_keys in (False, True):
        cfg = dict(E.LOOP, name='lstm_baseline', model_module_name='models.lstm_baseline', model_class_name='LSTMBaseline',
                   seed=1, embedding_size=8, hidden_size=16, n_layers=1, lr=1e-3, max_grad_norm=5, n_decay=1000)
        if with_keys:
            cfg.update(sample_temperature=1.0, sample_top_k=10, sample_seed=4, sample_primer_len=3, samples_per_episode=3)
        tmp = tmp_path / ('keys' if with_keys else 'plain')
        tmp.mkdir()
        p = E._write_configs(tmp, golden_dir, cfg)
        ck = str(tmp / 'ck')
        T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
        for i in range(cfg['n_samples']):
            files = sorted(os.listdir(os.path.join(ck, 'samples', 'sample_%d' % i)))
            if with_keys:
                assert files == ['model_sample_%d.txt' % j for j in range(3)] + ['support_%d.txt' % j for j in range(E.K)]
                texts = [open(os.path.join(ck, 'samples', 'sample_%d' % i, f)).read() for f in files[:3]]
                assert len(set(texts)) == 3
            else:
                assert files == ['model_sample.txt'] + ['support_%d.txt' % j for j in range(E.K)]
