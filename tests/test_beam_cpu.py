"""CPU checks of the numpy restatement of fsmg_beam_search (tests/beam_ref.py) that the GPU tests compare against, the ABI
symbols, and train.train's opt-in sample_beam_width key."""
import os
import re
import subprocess

import numpy as np

import beam_ref as BR
import gen_ref as R
from conftest import small_config
from oracle import lstm_oracle as O


def _tiny(input_size=4, H=12, L=2, seed=3):
    cfg = small_config(input_size=input_size, hidden_size=H, n_layers=L, embedding_size=6)
    params = O.glorot_init(cfg, seed)
    rng = np.random.RandomState(seed)
    params['softmax_b'] = rng.randn(*params['softmax_b'].shape)
    params['softmax_w'] = params['softmax_w'] * 4
    return cfg, params


def test_full_width_beam_is_exhaustive():
    # W = V1^(num-1): every prefix survives to the last position, so the W best are the W best of all V1^num sequences
    cfg, params = _tiny()
    V1, num = 5, 3
    W = V1 ** (num - 1)
    primer = np.array([[1, 3], [2, 0]])
    toks, scores, lps, _ = BR.beam_search(params, cfg, 2, W, num, primer=primer)
    for g in range(2):
        seqs, sc = BR.enumerate_all(params, cfg, num, primer[g])
        assert np.array_equal(toks[g], seqs[:W]), (toks[g], seqs[:W])
        assert np.allclose(scores[g], sc[:W], atol=1e-12)
        assert np.allclose(lps[g].sum(-1), scores[g], atol=1e-12)
        assert np.all(np.diff(scores[g]) <= 0)


def test_width_one_is_greedy():
    cfg, params = _tiny(input_size=30, H=10, L=1)
    primer = np.array([[4, 5, 6], [7, 8, 9]])
    toks, scores, lps, _ = BR.beam_search(params, cfg, 2, 1, 9, primer=primer)
    want, wlp = R.generate(params, cfg, 2, 9, temperature=0.0, primer=primer)
    assert np.array_equal(toks[:, 0], want)
    assert np.allclose(lps[:, 0], wlp, atol=1e-12)
    assert np.allclose(scores[:, 0], wlp.sum(-1), atol=1e-12)


def test_tie_rule_on_exact_ties():
    # s descending, then slot ascending, then logit descending, then column ascending; NaN below -inf
    lg = np.array([[1.0, 3.0, 2.0, 3.0], [1.0, 3.0, 2.0, 3.0]])
    order, s, _ = BR.rank([0.0, 0.0], lg)
    assert order[:6] == [(0, 1), (0, 3), (1, 1), (1, 3), (0, 2), (1, 2)]
    # the first position: slot 1 is dead (-inf) and ranks after every live candidate, its own in column order by logit
    order, _, _ = BR.rank([0.0, -np.inf], lg)
    assert order == [(0, 1), (0, 3), (0, 2), (0, 0), (1, 1), (1, 3), (1, 2), (1, 0)]
    # equal fp32 scores from different logits (lp rounds both to one value): the larger logit first, whatever its column
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2.0))
    lg32 = np.array([[b, a, -30.0]], np.float32)
    lse = np.array([np.float32(20.0)], np.float32)
    order, s, lp = BR.rank(np.array([0.0], np.float32), np.array([[a, b, -30.0]], np.float32), np.float32, lse=lse)
    assert s[0, 0] == s[0, 1] and order[:2] == [(0, 1), (0, 0)]
    order, _, _ = BR.rank(np.array([0.0], np.float32), lg32, np.float32, lse=lse)
    assert order[:2] == [(0, 0), (0, 1)]
    # NaN logits (and so NaN scores) rank below -inf ones; NaN among themselves by column
    lg = np.array([[np.nan, -np.inf, 0.5, np.nan]])
    order, _, _ = BR.rank([0.0], lg, lse=np.array([1.0]))
    assert order == [(0, 2), (0, 1), (0, 0), (0, 3)]
    # -0 ranks equal to +0: the column decides
    order, _, _ = BR.rank([0.0], np.array([[0.0, -0.0]]), lse=np.array([0.0]))
    assert order == [(0, 0), (0, 1)]
    order, _, _ = BR.rank([0.0], np.array([[-0.0, 0.0]]), lse=np.array([0.0]))
    assert order == [(0, 0), (0, 1)]


def test_scores_are_sums_and_groups_independent():
    cfg, params = _tiny(input_size=20, H=8, L=1)
    primer = np.array([[1, 2], [3, 4], [5, 6]])
    toks, scores, lps, gaps = BR.beam_search(params, cfg, 3, 4, 5, primer=primer)
    alone = BR.beam_search(params, cfg, 1, 4, 5, primer=primer[1:2])
    assert np.array_equal(toks[1], alone[0][0]) and np.array_equal(scores[1], alone[1][0])
    assert gaps.shape == (3, 5) and np.all(gaps > 0)
    for g in range(3):
        assert len({tuple(r) for r in toks[g]}) == 4
        for n in range(4):
            assert np.allclose(BR.sequence_logprobs(params, cfg, toks[g, n], primer[g]), lps[g, n], atol=1e-12)
    assert BR.fp32_sum([0.5, 0.25, -1.0]) == np.float32(-0.25)


def test_beam_symbols_bound_and_exported():
    from fsmg.build import build
    from fsmg.binding import SIGNATURES, library_path, load_library
    build()
    lib = load_library()
    for name in ('fsmg_beam_search', 'fsmg_maml_beam_search'):
        assert name in SIGNATURES
        getattr(lib, name)
    out = subprocess.check_output(['nm', '-D', '--defined-only', library_path()], universal_newlines=True)
    exported = set(re.findall(r' T (fsmg_[a-z_]+)$', out, flags=re.M))
    assert {'fsmg_beam_search', 'fsmg_maml_beam_search'} <= exported


def test_beam_config_layout_matches_header():
    import ctypes as C
    from fsmg.binding import FsmgBeamConfig, FSMG_BEAM_CONFIG_VERSION
    assert C.sizeof(FsmgBeamConfig) == 14 * 4
    from conftest import ROOT
    text = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert '#define FSMG_BEAM_CONFIG_VERSION %d' % FSMG_BEAM_CONFIG_VERSION in text


class FakeBeamModel(object):
    """a plugin with generate and beam_search (train.train's opt-in sample keys)"""
    calls = []

    def __init__(self, config):
        FakeBeamModel.calls = []

    def train(self, episode):
        return 1.0

    def eval(self, episode):
        return 1.0

    def save(self, checkpt_path):
        pass

    def recover_or_init(self, init_path):
        pass

    def sample(self, support_set, num):
        FakeBeamModel.calls.append(('sample', num))
        return [1] * num

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0):
        FakeBeamModel.calls.append(('generate', num, n))
        return np.arange(n * num).reshape(n, num) % 5

    def beam_search(self, support_set, num, beam_width, n=1, primer_len=0, logprobs=False):
        FakeBeamModel.calls.append(('beam_search', support_set.shape, num, beam_width, n, primer_len))
        toks = (np.arange(n * beam_width * num).reshape(n, beam_width, num) % 7).astype(np.int32)
        return toks, -np.arange(1, n * beam_width + 1, dtype=np.float32).reshape(n, beam_width) / 4


def _run(tmp_path, golden_dir, extra):
    import test_train_entry as E
    import train.train as T
    cfg = dict(E.LOOP, name='fake', model_module_name='test_beam_cpu', model_class_name='FakeBeamModel', **extra)
    tmp = tmp_path / ('run%d' % len(os.listdir(str(tmp_path))))
    tmp.mkdir()
    p = E._write_configs(tmp, golden_dir, cfg)
    ck = str(tmp / 'ck')
    T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
    files = [sorted(os.listdir(os.path.join(ck, 'samples', 'sample_%d' % i))) for i in range(cfg['n_samples'])]
    return ck, files, list(FakeBeamModel.calls)


def test_train_entry_sample_beam_width_with_a_fake_plugin(tmp_path, golden_dir):
    import test_train_entry as E
    support = ['support_%d.txt' % j for j in range(E.K)]
    beams = ['beam_scores.txt'] + ['model_beam_%d.txt' % j for j in range(3)]
    # without the key: the files of today, whatever the sample_temperature keys say
    _, files, calls = _run(tmp_path, golden_dir, {})
    assert files == [['model_sample.txt'] + support] * E.LOOP['n_samples']
    assert all(c[0] == 'sample' for c in calls)
    _, files, calls = _run(tmp_path, golden_dir, dict(sample_temperature=0.8, samples_per_episode=2))
    assert files == [['model_sample_0.txt', 'model_sample_1.txt'] + support] * E.LOOP['n_samples']
    assert not [c for c in calls if c[0] == 'beam_search']
    # with it: the beam's hypotheses best first and their scores, primed by sample_primer_len, beside today's sample
    ck, files, calls = _run(tmp_path, golden_dir, dict(sample_beam_width=3, sample_primer_len=2))
    assert files == [sorted(beams + ['model_sample.txt'] + support)] * E.LOOP['n_samples']
    assert [c for c in calls if c[0] == 'beam_search'] == [('beam_search', (E.K, E.MAXLEN), E.MAXLEN, 3, 1, 2)] * E.LOOP['n_samples']
    d = os.path.join(ck, 'samples', 'sample_0')
    assert [float(x) for x in open(os.path.join(d, 'beam_scores.txt')).read().split()] == [-0.25, -0.5, -0.75]
    texts = [open(os.path.join(d, 'model_beam_%d.txt' % j)).read() for j in range(3)]
    assert len(set(texts)) == 3
    _, files, calls = _run(tmp_path, golden_dir, dict(sample_beam_width=3, sample_temperature=1.0, samples_per_episode=2))
    assert files == [sorted(beams + ['model_sample_0.txt', 'model_sample_1.txt'] + support)] * E.LOOP['n_samples']
