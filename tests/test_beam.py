"""fsmg_beam_search / fsmg_maml_beam_search on the MI355X against the fp64 numpy restatement (tests/beam_ref.py): exhaustive
search on tiny models, hypotheses and their order where the fp64 gaps are clear, the boundary tie rule, greedy parity at W = 1,
determinism and group independence, large vocabularies, NaN logits, no side effects, errors, and the plugin / train.train
surface."""
import ctypes as C
import os

import numpy as np
import pytest

import beam_ref as BR
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _trained(cfg, steps=3, seed=7, **kw):
    m = new_model(cfg, **kw)
    for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
        m.train_step(sup, qry)
    return m


def _check_invariants(params, cfg, toks, scores, lps, primer=None, hyps=None):
    """distinct, best first, score == fp32 sum of lps bitwise, every token in range, each lp within TOL of fp64"""
    G, W, num = toks.shape
    V1 = cfg['input_size'] + 1
    assert np.all((toks >= 0) & (toks < V1))
    for g in range(G):
        assert len({tuple(r) for r in toks[g]}) == W, ('not distinct', g)
        assert np.all(np.diff(scores[g].astype(np.float64)) <= 0), ('not sorted', g, scores[g])
        for n in range(W):
            assert BR.fp32_sum(lps[g, n]).view(np.uint32) == np.float32(scores[g, n]).view(np.uint32), (g, n)
        for n in (range(W) if hyps is None else hyps):
            want = BR.sequence_logprobs(params, cfg, toks[g, n], None if primer is None else primer[g])
            assert np.max(np.abs(lps[g, n] - want)) <= TOL, (g, n, lps[g, n], want)
            assert abs(float(scores[g, n]) - want.sum()) <= TOL * num, (g, n)


def _matches_reference(params, cfg, toks, scores, G, W, num, primer=None):
    """-> number of groups whose fp64 gaps all exceed TOL (each of those must equal the reference's hypotheses and order)"""
    rt, rs, _, gaps = BR.beam_search(params, cfg, G, W, num, primer=primer)
    clear = 0
    for g in range(G):
        if np.all(gaps[g] > TOL):
            clear += 1
            assert np.array_equal(toks[g], rt[g]), (g, toks[g], rt[g])
            assert np.max(np.abs(scores[g] - rs[g])) <= TOL * num
    return clear


@pytest.mark.parametrize('input_size,L', [(4, 1), (4, 2), (7, 1), (7, 2)])
def test_exhaustive_on_tiny_models(input_size, L):
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16, n_layers=L)
    m = _trained(cfg)
    params = f64_params(m)
    V1, num = input_size + 1, 3
    W = V1 ** 2
    primer = np.array([[1, 2], [3, 0]], np.int32)
    for G, pr in ((1, None), (2, primer)):
        toks, scores, lps = m.beam_search(num, W, n_groups=G, primer=pr, logprobs=True)
        assert toks.shape == (G, W, num) and scores.shape == (G, W) and lps.shape == (G, W, num)
        _check_invariants(params, cfg, toks, scores, lps, primer=pr)
        for g in range(G):
            seqs, sc = BR.enumerate_all(params, cfg, num, None if pr is None else pr[g])
            want = {tuple(q) for q in seqs[:W]}
            got = {tuple(q) for q in toks[g]}
            boundary = sc[W - 1] - sc[W] if W < len(sc) else np.inf
            if boundary > TOL:
                assert got == want, (g, got ^ want)
            else:      # only hypotheses whose fp64 score is within TOL of the boundary may trade places
                for q in got ^ want:
                    i = [tuple(x) for x in seqs].index(q)
                    assert abs(sc[i] - sc[W - 1]) <= TOL, (g, q, sc[i], sc[W - 1])


@pytest.mark.parametrize('H,L', [(24, 1), (200, 2), (512, 1), (1024, 2)])
def test_against_reference_across_hidden_sizes(H, L):
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)
    m = _trained(cfg)
    # a wider spread of state-dependent logits than a briefly trained model has: clear gaps between adjacent ranks
    m.set_param('softmax_w', m.get_param('softmax_w') * 40)
    m.set_param('softmax_b', (np.random.RandomState(H).randn(301) * 2).astype(np.float32))
    params = f64_params(m)
    num = 4
    clear = total = 0
    for G, W, P in ((3, 4, 0), (2, 16, 4), (2, 64, 0), (3, 4, 6), (2, 16, 0), (2, 64, 3)):
        primer = np.random.RandomState(G * W + P).randint(0, 300, size=(G, P)).astype(np.int32) if P else None
        toks, scores, lps = m.beam_search(num, W, n_groups=G, primer=primer, logprobs=True)
        _check_invariants(params, cfg, toks, scores, lps, primer=primer, hyps=range(0, W, max(1, W // 8)))
        clear += _matches_reference(params, cfg, toks, scores, G, W, num, primer=primer)
        total += G
    assert 2 * clear >= total, (clear, total)


@pytest.mark.parametrize('which', ['cfg-B', 'cfg-C'])
def test_full_size(which):
    if which == 'cfg-B':
        cfg = small_config(input_size=10000, max_len=32, embedding_size=250, hidden_size=512, n_layers=1)
    else:
        cfg = small_config(input_size=4708, max_len=32, embedding_size=250, hidden_size=1024, n_layers=2)
    m = _trained(cfg, steps=2)
    params = f64_params(m)
    primer = np.random.RandomState(2).randint(0, cfg['input_size'], size=(4, 3)).astype(np.int32)
    toks, scores, lps = m.beam_search(32, 16, n_groups=4, primer=primer, logprobs=True)
    _check_invariants(params, cfg, toks, scores, lps, primer=primer, hyps=(0, 7, 15))


def test_exact_ties_follow_the_rule():
    # zero weights: every row's logits are softmax_b, whose values repeat; within a row the ties are exact on the device and in
    # fp64 alike, and the pair sums of four distinct values are distinct, so the order is the tie rule's (staged and unstaged rows)
    for input_size, W in ((40, 8), (40, 16), (40000, 8)):
        cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
        m = new_model(cfg)
        params = {k: np.zeros_like(v) for k, v in m.get_params().items()}
        params['softmax_b'] = np.random.RandomState(input_size).choice(
            np.array([0.3, 1.1, -0.4, 2.2], np.float32), input_size + 1).astype(np.float32)
        m.set_params(params)
        toks, scores = m.beam_search(2, W, n_groups=2)
        rt, _, _, _ = BR.beam_search(f64_params(m), cfg, 2, W, 2)
        assert np.array_equal(toks, rt), (input_size, W, toks, rt)


@pytest.mark.parametrize('G', [1, 7])
def test_width_one_is_greedy_generate_bitwise(G):
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=48, n_layers=2)
    m = _trained(cfg)
    for primer in (None, np.random.RandomState(G).randint(0, 97, size=(G, 5)).astype(np.int32)):
        toks, scores, lps = m.beam_search(24, 1, n_groups=G, primer=primer, logprobs=True)
        want, wlp = m.generate(G, 24, temperature=0.0, primer=primer, logprobs=True)
        assert np.array_equal(toks[:, 0], want)
        assert np.array_equal(lps[:, 0].view(np.uint32), wlp.view(np.uint32))
        for g in range(G):
            assert BR.fp32_sum(wlp[g]).view(np.uint32) == scores[g, 0].view(np.uint32)


def test_determinism_and_group_independence():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=64, n_layers=2)
    m = _trained(cfg)
    primer = np.random.RandomState(0).randint(0, 97, size=(9, 4)).astype(np.int32)
    a = m.beam_search(10, 16, n_groups=9, primer=primer, logprobs=True)
    b = m.beam_search(10, 16, n_groups=9, primer=primer, logprobs=True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for g in (0, 4, 8):
        alone = m.beam_search(10, 16, n_groups=1, primer=primer[g:g + 1], logprobs=True)
        for x, y in zip(a, alone):
            assert np.array_equal(x[g].view(np.uint32), y[0].view(np.uint32)), g
    c = m.beam_search(10, 16, n_groups=3, primer=primer[3:6], logprobs=True)
    for x, y in zip(a, c):
        assert np.array_equal(x[3:6].view(np.uint32), y.view(np.uint32))


def test_large_vocabulary_unstaged_rows():
    # V1 = 40 001 > 32 768: the row top-W reads the logits from global memory
    cfg = small_config(input_size=40000, max_len=8, embedding_size=8, hidden_size=16)
    m = _trained(cfg, steps=1)
    params = f64_params(m)
    primer = np.array([[5, 17], [39999, 0]], np.int32)
    toks, scores, lps = m.beam_search(4, 8, n_groups=2, primer=primer, logprobs=True)
    _check_invariants(params, cfg, toks, scores, lps, primer=primer)
    _matches_reference(params, cfg, toks, scores, 2, 8, 4, primer=primer)


@pytest.mark.parametrize('input_size', [97, 40000])
def test_nan_logits_give_in_range_tokens(input_size):
    cfg = small_config(input_size=input_size, max_len=8, embedding_size=8, hidden_size=16)
    m = new_model(cfg)
    m.set_param('softmax_b', np.full(input_size + 1, np.nan, np.float32))
    for W in (1, 4, 16):
        toks, scores = m.beam_search(5, W, n_groups=3, primer=np.full((3, 2), 3, np.int32))
        assert np.all((toks >= 0) & (toks <= input_size)), (W, toks)
    m.set_param('softmax_b', np.zeros(input_size + 1, np.float32))
    toks, scores = m.beam_search(4, 4, n_groups=2)                 # the handle stays usable
    assert np.all((toks >= 0) & (toks <= input_size)) and np.all(np.isfinite(scores))


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


def test_beam_search_changes_no_state():
    cfg = small_config(input_size=97, max_len=12, embedding_size=12, hidden_size=32)
    sup, qry = O.synthetic_episodes(1, 2, 2, 2, 12, 97, seed=3)[0]
    m1, m2 = _trained(cfg), _trained(cfg)
    m1.forward_backward(sup, qry)
    m2.forward_backward(sup, qry)
    grads = {k: m1.get_grad(k) for k in m1.param_shapes}
    before = _state(m1)
    m1.beam_search(15, 8, n_groups=3, primer=np.ones((3, 2), np.int32))
    _same_state(before, _state(m1))
    for k, v in grads.items():
        assert np.array_equal(v.view(np.uint32), m1.get_grad(k).view(np.uint32)), k
    l1, l2 = m1.apply_update(), m2.apply_update()
    assert l1 == l2
    for k, v in m1.get_params().items():
        assert np.array_equal(v, m2.get_param(k)), k


def test_maml_beam_search_adapts_restores_and_matches_oracle():
    cfg = small_config(input_size=60, max_len=10, embedding_size=10, hidden_size=32)
    m = _trained(cfg)
    support = np.random.RandomState(4).randint(0, 60, size=(3, 10)).astype(np.int32)
    theta = m.get_params()
    b0 = m.beam_search(8, 8, n_groups=2)
    toks, scores, lps = m.maml_beam_search(support, 8, 2, 0.1, 8, n_groups=2, logprobs=True)
    for k, v in m.get_params().items():
        assert np.array_equal(v.view(np.uint32), theta[k].view(np.uint32)), k
    fast, _ = O.maml_adapt({k: v.astype(np.float64) for k, v in theta.items()}, support[None], cfg, inner_steps=2, inner_lr=0.1)
    _check_invariants(fast, cfg, toks, scores, lps)
    _matches_reference(fast, cfg, toks, scores, 2, 8, 8)
    b1 = m.beam_search(8, 8, n_groups=2)
    assert np.array_equal(b0[0], b1[0]) and np.array_equal(b0[1].view(np.uint32), b1[1].view(np.uint32))
    assert not np.array_equal(scores, b0[1])


def test_argument_errors():
    from fsmg.binding import FsmgError
    cfg = small_config(input_size=3, max_len=8, embedding_size=8, hidden_size=16)     # V1 = 4
    m = new_model(cfg)
    toks = np.full((2, 64, 40), -5, np.int32)          # room for the largest valid call below
    scores = np.full((2, 64), -5, np.float32)

    def call(primer=None, **over):
        b = m.beam_config(2, 4, 2)
        for k, v in over.items():
            if k == 'reserved':
                b.reserved[v] = 1
            else:
                setattr(b, k, v)
        return m._lib.fsmg_beam_search(m._h, C.byref(b), primer, toks.ctypes.data_as(C.POINTER(C.c_int32)),
                                       scores.ctypes.data_as(C.POINTER(C.c_float)), None)

    assert call() == 0
    assert call(beam_width=16) == 0 and call(beam_width=64, num=3) == 0          # W == V1^num
    for bad in (dict(version=2), dict(reserved=0), dict(reserved=7), dict(n_groups=0), dict(n_groups=-3), dict(beam_width=0),
                dict(beam_width=65), dict(beam_width=17), dict(beam_width=5, num=1), dict(num=0), dict(num=-1),
                dict(primer_len=-1), dict(primer_len=2), dict(primer_on_device=2), dict(n_groups=1 << 16, beam_width=64)):
        assert call(**bad) == -1, bad
    assert m._lib.fsmg_beam_search(m._h, C.byref(m.beam_config(1, 2, 2)), None, None,
                                   scores.ctypes.data_as(C.POINTER(C.c_float)), None) == -1
    assert m._lib.fsmg_beam_search(m._h, C.byref(m.beam_config(1, 2, 2)), None, toks.ctypes.data_as(C.POINTER(C.c_int32)),
                                   None, None) == -1
    # a large num with W <= V1^num (no overflow in the check)
    assert call(beam_width=64, num=40) == 0
    # primer ids outside [0, input_size): host and device, outputs unwritten
    t0, s0 = toks.copy(), scores.copy()
    with pytest.raises(FsmgError) as e:
        m.beam_search(2, 2, n_groups=2, primer=np.array([[1, 3], [0, 0]]))
    assert e.value.code == -7
    import torch
    dp = torch.tensor([[1, 2], [0, -1]], dtype=torch.int32, device='cuda')
    bad = m.beam_config(2, 2, 2, 2, 1)
    assert m._lib.fsmg_beam_search(m._h, C.byref(bad), C.c_void_p(dp.data_ptr()), toks.ctypes.data_as(C.POINTER(C.c_int32)),
                                   scores.ctypes.data_as(C.POINTER(C.c_float)), None) == -7
    assert np.array_equal(toks, t0) and np.array_equal(scores, s0)
    dp[1, 1] = 2
    host = m.beam_search(3, 4, n_groups=2, primer=np.array([[1, 2], [0, 2]]))
    dev = m.beam_search(3, 4, n_groups=2, primer=(dp.data_ptr(), 2))
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    # the MAML entry: a bad config first, then bad support arguments
    support = np.zeros((2, 8), np.int32)
    with pytest.raises(FsmgError) as e:
        m.maml_beam_search(support, 2, 1, 0.1, 65)
    assert e.value.code == -1
    with pytest.raises(FsmgError) as e:
        m.maml_beam_search(support, 2, 65, 0.1, 2)
    assert e.value.code == -1
    with pytest.raises(FsmgError) as e:
        m.maml_beam_search(support, 2, 1, float('nan'), 2)
    assert e.value.code == -1


def _plugin_cfg(tmp, name='lstm_baseline'):
    return dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name=name,
                checkpt_dir=str(tmp), inner_steps=1, inner_lr=0.1)


def test_plugin_beam_search(tmp_path):
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    support = np.random.RandomState(5).randint(0, 40, size=(3, 12)).astype(np.int32)
    for cls in (LSTMBaseline, MAMLLSTM):
        model = cls(_plugin_cfg(tmp_path / cls.__name__, cls.__name__.lower()))
        model.recover_or_init('')
        toks, scores = model.beam_search(support, 10, 6, n=5, primer_len=4)
        assert toks.shape == (5, 6, 10) and toks.dtype == np.int32 and scores.shape == (5, 6)
        again = model.beam_search(support, 10, 6, n=5, primer_len=4)
        assert np.array_equal(toks, again[0]) and np.array_equal(scores, again[1])
        t, s, lp = model.beam_search(support, 10, 6, n=5, primer_len=4, logprobs=True)
        assert np.array_equal(t, toks) and lp.shape == (5, 6, 10)
        if cls is LSTMBaseline:
            # the primer is the support songs' first tokens, dealt round-robin; W = 1 is the greedy draw of generate
            want = model.engine.beam_search(10, 6, n_groups=5, primer=support[np.arange(5) % 3, :4])
            assert np.array_equal(toks, want[0])
            g = model.generate(support, 7, n=2, temperature=0.0, primer_len=2)
            assert np.array_equal(model.beam_search(support, 7, 1, n=2, primer_len=2)[0][:, 0], g)
        else:
            # searched at theta' adapted on the support set: the scores differ from the unadapted search's
            _, s0 = LSTMBaseline.beam_search(model, support, 10, 6, n=5, primer_len=4)
            assert not np.array_equal(scores, s0)


def test_train_entry_with_sample_beam_width(tmp_path, golden_dir):
    import test_train_entry as E
    import train.train as T
    for with_key in (False, True):
        cfg = dict(E.LOOP, name='lstm_baseline', model_module_name='models.lstm_baseline', model_class_name='LSTMBaseline',
                   seed=1, embedding_size=8, hidden_size=16, n_layers=1, lr=1e-3, max_grad_norm=5, n_decay=1000)
        if with_key:
            cfg.update(sample_beam_width=4, sample_primer_len=3)
        tmp = tmp_path / ('key' if with_key else 'plain')
        tmp.mkdir()
        p = E._write_configs(tmp, golden_dir, cfg)
        ck = str(tmp / 'ck')
        T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
        for i in range(cfg['n_samples']):
            d = os.path.join(ck, 'samples', 'sample_%d' % i)
            files = sorted(os.listdir(d))
            base = ['model_sample.txt'] + ['support_%d.txt' % j for j in range(E.K)]
            if with_key:
                assert files == sorted(base + ['beam_scores.txt'] + ['model_beam_%d.txt' % j for j in range(4)])
                sc = [float(x) for x in open(os.path.join(d, 'beam_scores.txt')).read().split()]
                assert len(sc) == 4 and sc == sorted(sc, reverse=True) and all(np.isfinite(sc))
                texts = [open(os.path.join(d, 'model_beam_%d.txt' % j)).read() for j in range(4)]
                assert len(set(texts)) == 4
            else:
                assert files == base
