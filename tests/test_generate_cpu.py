"""CPU checks of the numpy restatement of fsmg_generate (tests/gen_ref.py) that the GPU tests compare against."""
import numpy as np

import gen_ref as R
from conftest import small_config
from oracle import lstm_oracle as O


def test_philox4x32_10_known_answers():
    # Random123 known-answer vectors (kat_vectors, philox4x32_10)
    cases = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, out in cases:
        got = R.philox4x32_10(np.array([ctr], np.uint64), key)[0]
        assert [int(x) for x in got] == list(out), [hex(int(x)) for x in got]


def test_gumbel_noise_counter_layout():
    # word v & 3 of the block at counter (v >> 2, t, b, 0); the counter does not depend on the row count
    g = R.gumbel(0x123456789, 3, 5, 11)
    x = R.philox4x32_10(np.array([[2, 3, 5, 0]], np.uint64), (0x23456789, 0x1))[0]
    u = ((int(x[1]) >> 8) + 0.5) * 2.0 ** -24
    assert g[9] == -np.log(-np.log(u))
    assert np.all(np.isfinite(g))


def test_reference_greedy_decode_equals_oracle_sample():
    cfg = small_config(input_size=40, hidden_size=12, n_layers=2, embedding_size=6)
    params = O.glorot_init(cfg, 3)
    params['bias_0'] = np.random.RandomState(0).randn(*params['bias_0'].shape)
    params['softmax_b'] = np.random.RandomState(1).randn(*params['softmax_b'].shape)
    toks, lps = R.generate(params, cfg, 3, 12, temperature=0.0)
    want = O.sample(params, 12, cfg)
    for b in range(3):
        assert list(toks[b]) == want
    assert np.all(lps <= 0)
    assert R.check_margins(params, cfg, toks, lps, 0.0, 0, 0) == 0


def test_reference_sampling_restricts_to_top_k_and_depends_on_seed():
    cfg = small_config(input_size=30, hidden_size=8)
    params = O.glorot_init(cfg, 5)
    params['softmax_b'] = np.random.RandomState(2).randn(*params['softmax_b'].shape) * 2
    primer = np.array([[1, 2, 3], [4, 5, 6]])
    t1, l1 = R.generate(params, cfg, 2, 16, temperature=1.0, top_k=3, seed=7, primer=primer)
    t2, _ = R.generate(params, cfg, 2, 16, temperature=1.0, top_k=3, seed=8, primer=primer)
    assert not np.array_equal(t1, t2)
    R.check_margins(params, cfg, t1, l1, 1.0, 3, 7, primer=primer)


class FakeGenModel(object):
    """a plugin with generate (train.train's opt-in sample keys)"""
    calls = []

    def __init__(self, config):
        FakeGenModel.calls = []

    def train(self, episode):
        return 1.0

    def eval(self, episode):
        return 1.0

    def save(self, checkpt_path):
        pass

    def recover_or_init(self, init_path):
        pass

    def sample(self, support_set, num):
        FakeGenModel.calls.append(('sample', num))
        return [1] * num

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0):
        FakeGenModel.calls.append(('generate', support_set.shape, num, n, temperature, top_k, seed, primer_len))
        return np.arange(n * num).reshape(n, num) % 5


def test_train_entry_sample_keys_with_a_fake_plugin(tmp_path, golden_dir):
    import os
    import test_train_entry as E
    import train.train as T
    seen = {}
    for with_keys in (False, True):
        cfg = dict(E.LOOP, name='fake', model_module_name='test_generate_cpu', model_class_name='FakeGenModel')
        if with_keys:
            cfg.update(sample_temperature=0.8, sample_top_k=4, sample_seed=9, sample_primer_len=2, samples_per_episode=3)
        tmp = tmp_path / str(with_keys)
        tmp.mkdir()
        p = E._write_configs(tmp, golden_dir, cfg)
        ck = str(tmp / 'ck')
        T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
        calls = [c for c in FakeGenModel.calls if c[0] in ('sample', 'generate')]
        seen[with_keys] = calls
        for i in range(cfg['n_samples']):
            files = sorted(os.listdir(os.path.join(ck, 'samples', 'sample_%d' % i)))
            want = ['model_sample_%d.txt' % j for j in range(3)] if with_keys else ['model_sample.txt']
            assert files == want + ['support_%d.txt' % j for j in range(E.K)]
    assert seen[False] == [('sample', E.MAXLEN)] * E.LOOP['n_samples']
    gens = seen[True]
    assert [c[:6] for c in gens] == [('generate', (E.K, E.MAXLEN), E.MAXLEN, 3, 0.8, 4)] * E.LOOP['n_samples']
    assert all(c[7] == 2 for c in gens)
    seeds = [c[6] for c in gens]
    assert len(set(seeds)) == len(seeds) and seeds[0] == T.sample_seed(9, 0)
