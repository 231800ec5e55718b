"""CPU checks of the numpy restatement of fsmg_generate_filtered (tests/filter_ref.py) that the GPU tests compare against, and of
train.train's opt-in sampling-filter keys with a fake plugin."""
import numpy as np
import pytest

import filter_ref as F
import gen_ref as R
from conftest import small_config
from oracle import lstm_oracle as O

LN2 = np.log(2.0)


def brute_final(zp, T, top_k, top_p, min_p):
    """steps 2-4 by sorting: the final set as a bool mask (T > 0)"""
    V1 = zp.size
    keep = [v for v in range(V1) if not np.isnan(zp[v])]
    if top_k not in (0, V1):
        srt = sorted((zp[v] for v in keep), reverse=True)
        if len(srt) >= top_k:
            keep = [v for v in keep if zp[v] >= srt[top_k - 1]]
    if not keep:
        return np.zeros(V1, bool)
    zmax = max(zp[v] for v in keep)
    rel = {v: 0.0 if zp[v] == zmax else (zp[v] - zmax) / T for v in keep}
    if min_p > 0:
        keep = [v for v in keep if rel[v] >= np.log(min_p)]
    if 0 < top_p < 1:
        order = sorted(keep, key=lambda v: -zp[v])
        w = np.array([np.exp(rel[v]) for v in order])
        q = w / w.sum()
        cum, out, i = 0.0, [], 0
        while i < len(order):          # one group of equal z' at a time: its mass-ahead is the sum of the groups before it
            j = i
            while j < len(order) and zp[order[j]] == zp[order[i]]:
                j += 1
            if cum < top_p:
                out += order[i:j]
            cum += q[i:j].sum()
            i = j
        keep = out
    m = np.zeros(V1, bool)
    m[keep] = True
    return m


def test_final_set_matches_sort_and_cumsum_on_random_vectors():
    rs = np.random.RandomState(0)
    for trial in range(300):
        V1 = int(rs.randint(2, 60))
        z = rs.randn(V1) * rs.choice([0.3, 1.0, 4.0])
        if trial % 3 == 0:
            z = np.round(z, 1)                  # many ties
        if trial % 5 == 0:
            z[rs.randint(V1)] = -np.inf
        if trial % 7 == 0:
            z[rs.randint(V1)] = np.nan
        T = float(rs.choice([0.5, 1.0, 2.0]))
        k = int(rs.choice([0, 0, 1, 3, V1, min(V1, 7)]))
        p = float(rs.choice([0.0, 0.05, 0.5, 0.9, 0.999, 1.0]))
        m = float(rs.choice([0.0, 0.01, 0.2, 1.0]))
        ctx = rs.randint(0, V1, size=rs.randint(0, 10))
        zp = F.penalise(z, ctx, float(rs.choice([1.0, 0.5, 1.5, 1e6])), int(rs.choice([0, 1, 4, 20])))
        if k == 1:
            continue
        s = F.filter_sets(zp, T, k, p, m)
        assert np.array_equal(s['F'], brute_final(zp, T, k, p, m)), (trial, zp, T, k, p, m)
        comp = ~np.isnan(zp)
        if comp.any():
            assert s['F'][F.argmax_comparable(zp)], trial          # the top column always stays


def test_top_p_boundary_ties_and_mass_exactly_at_p():
    # weights 1, 1/2, 1/4, 1/4 (T = 1): q = .5, .25, .125, .125, all exact in fp64
    zp = np.array([0.0, -LN2, -2 * LN2, -2 * LN2, -np.inf])
    cases = {0.5: [0], 0.5 + 1e-12: [0, 1], 0.75: [0, 1], 0.75 + 1e-12: [0, 1, 2, 3], 1e-9: [0], 0.9999: [0, 1, 2, 3]}
    for p, want in cases.items():
        s = F.filter_sets(zp, 1.0, 0, p, 0.0)
        assert np.flatnonzero(s['F']).tolist() == want, (p, np.flatnonzero(s['F']))
        assert np.array_equal(s['F'], brute_final(zp, 1.0, 0, p, 0.0)), p
    # a tie at the top: both stay even for a tiny p
    s = F.filter_sets(np.array([1.0, 3.0, 3.0, 2.0]), 1.0, 0, 1e-6, 0.0)
    assert np.flatnonzero(s['F']).tolist() == [1, 2]


def test_min_p_boundary_and_temperature():
    zp = np.array([0.0, -LN2, -2 * LN2, -3.0, np.nan])
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 0, 0.0, 0.5)['F']).tolist() == [0, 1]       # q_v / q_max = 1/2 >= 1/2
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 0, 0.0, 0.25)['F']).tolist() == [0, 1, 2]
    assert np.flatnonzero(F.filter_sets(zp, 2.0, 0, 0.0, 0.5)['F']).tolist() == [0, 1, 2]    # T = 2 flattens
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 0, 0.0, 1.0)['F']).tolist() == [0]
    # min-p then top-p renormalised over the min-p survivors: q = 2/3, 1/3
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 0, 0.6, 0.5)['F']).tolist() == [0]
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 0, 0.7, 0.5)['F']).tolist() == [0, 1]


def test_top_k_first_then_min_p_and_top_p():
    zp = np.array([3.0, 2.0, 2.0, 1.0, 0.0])
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 2, 0.0, 0.0)['F']).tolist() == [0, 1, 2]       # ties at the top-k boundary
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 4, 0.0, 0.2)['F']).tolist() == [0, 1, 2]       # e^-2 < 0.2 <= e^-1
    assert np.flatnonzero(F.filter_sets(zp, 1.0, 4, 0.99, 0.0)['F']).tolist() == [0, 1, 2, 3]
    # NaN never counts among the top k: with fewer comparable columns than k, all of them stay
    zn = np.array([np.nan, 1.0, np.nan, 0.5])
    assert np.flatnonzero(F.filter_sets(zn, 1.0, 3, 0.0, 0.0)['F']).tolist() == [1, 3]


def test_non_finite_columns():
    noise = np.zeros(5)
    # +inf: only the +inf columns survive min-p / top-p, and they have all the mass
    zi = np.array([1.0, np.inf, 0.0, np.inf, np.nan])
    assert np.flatnonzero(F.filter_sets(zi, 1.0, 0, 0.5, 0.0)['F']).tolist() == [1, 3]
    assert np.flatnonzero(F.filter_sets(zi, 1.0, 0, 0.0, 0.1)['F']).tolist() == [1, 3]
    # -inf columns are comparable: drawn (lowest index) rather than a NaN column when nothing else is there
    zm = np.array([np.nan, -np.inf, np.nan, -np.inf])
    for p, m in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.9, 0.1)):
        assert F.choose(zm, 1.0, 0, p, m, np.zeros(4))[0] == 1
    assert F.choose(zm, 0.0, 0, 0.0, 0.0, np.zeros(4))[0] == 1
    # no comparable column at all: column 0
    assert F.choose(np.full(5, np.nan), 1.0, 0, 0.5, 0.1, noise)[0] == 0
    assert F.choose(np.full(5, np.nan), 0.0, 0, 0.5, 0.1, noise)[0] == 0


def test_penalty_rule_and_window():
    z = np.array([2.0, -1.0, 0.0, 4.0, np.nan, -3.0])
    ctx = [1, 3, 3, 4, 0]
    p = F.penalise(z, ctx, 2.0, 0)
    assert p[0] == 1.0 and p[1] == -2.0 and p[3] == 2.0 and np.isnan(p[4]) and p[2] == 0.0 and p[5] == -3.0
    p = F.penalise(z, ctx, 0.5, 0)          # theta < 1 rewards instead
    assert p[0] == 4.0 and p[1] == -0.5 and p[3] == 8.0
    p = F.penalise(z, ctx, 2.0, 2)          # the last two context tokens only: 4 and 0
    assert p[0] == 1.0 and p[1] == -1.0 and p[3] == 4.0
    p = F.penalise(z, ctx, 2.0, 100)        # a window longer than the context: all of it
    assert np.array_equal(p, F.penalise(z, ctx, 2.0, 0), equal_nan=True)
    assert np.array_equal(F.penalise(z, [], 2.0, 3), z, equal_nan=True)
    assert np.array_equal(F.penalise(z, ctx, 1.0, 0), z, equal_nan=True)
    assert np.array_equal(F.penalise(z, ctx, 0.0, 0), z, equal_nan=True)
    # once per id however often it occurs
    assert F.penalise(np.array([8.0]), [0, 0, 0], 2.0, 0)[0] == 4.0


def test_neutral_reference_equals_gen_ref_choose():
    rs = np.random.RandomState(3)
    for trial in range(200):
        V1 = int(rs.randint(2, 50))
        z = rs.randn(V1) * 3
        T = float(rs.choice([0.0, 0.7, 1.0, 2.0]))
        k = int(rs.choice([0, 1, 3, V1]))
        noise = rs.gumbel(size=V1)
        want, _ = R.choose(z, T, k, noise)
        for p, m, th in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)):
            assert F.neutral(p, m, th)
            zp = F.penalise(z, rs.randint(0, V1, size=5), th, 0)
            assert F.choose(zp, T, k, p, m, noise)[0] == want, trial


def test_reference_decoder_filters_and_margins():
    cfg = small_config(input_size=30, hidden_size=8)
    params = O.glorot_init(cfg, 5)
    params['softmax_b'] = np.random.RandomState(2).randn(*params['softmax_b'].shape) * 2
    primer = np.array([[1, 2, 3], [4, 5, 6]])
    t0, l0 = R.generate(params, cfg, 2, 12, temperature=1.0, top_k=3, seed=7, primer=primer)
    t1, l1 = F.generate(params, cfg, 2, 12, temperature=1.0, top_k=3, seed=7, primer=primer)
    assert np.array_equal(t0, t1) and np.allclose(l0, l1)
    kw = dict(temperature=0.8, top_k=0, seed=7, primer=primer, top_p=0.8, min_p=0.05, theta=1.5, window=4)
    t2, l2 = F.generate(params, cfg, 2, 12, **kw)
    F.check_margins(params, cfg, t2, l2, kw['temperature'], 0, 7, top_p=0.8, min_p=0.05, theta=1.5, window=4, primer=primer)
    # greedy with a huge penalty never repeats an id inside the window
    t3, _ = F.generate(params, cfg, 1, 10, temperature=0.0, theta=1e6, window=5)
    for t in range(10):
        assert t3[0, t] not in t3[0, max(0, t - 5):t]


class FakeFilterModel(object):
    """a plugin whose generate takes the sampling-filter keywords (train.train's opt-in sample_* keys)"""
    calls = []

    def __init__(self, config):
        FakeFilterModel.calls = []

    def train(self, episode):
        return 1.0

    def eval(self, episode):
        return 1.0

    def save(self, checkpt_path):
        pass

    def recover_or_init(self, init_path):
        pass

    def sample(self, support_set, num):
        return [1] * num

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0, **filters):
        FakeFilterModel.calls.append(('generate', n, temperature, top_k, primer_len, filters))
        return np.arange(n * num).reshape(n, num) % 5


@pytest.mark.parametrize('keys', ['none', 'some', 'all'])
def test_train_entry_passes_filter_keys(tmp_path, golden_dir, keys):
    import os
    import test_train_entry as E
    import train.train as T
    cfg = dict(E.LOOP, name='fake', model_module_name='test_generate_filters_cpu', model_class_name='FakeFilterModel',
               sample_temperature=0.8, sample_top_k=4, samples_per_episode=2)
    want = {}
    if keys in ('some', 'all'):
        cfg.update(sample_top_p=0.9, sample_repeat_window=16)
        want.update(top_p=0.9, repeat_window=16)
    if keys == 'all':
        cfg.update(sample_min_p=0.05, sample_repetition_penalty=1.2)
        want.update(min_p=0.05, repetition_penalty=1.2)
    p = E._write_configs(tmp_path, golden_dir, cfg)
    ck = str(tmp_path / 'ck')
    T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
    gens = [c for c in FakeFilterModel.calls if c[0] == 'generate']
    assert len(gens) == E.LOOP['n_samples']
    for c in gens:
        assert c[1:5] == (2, 0.8, 4, 0) and c[5] == want, c
        assert all(type(v) is (int if k == 'repeat_window' else float) for k, v in c[5].items())
    for i in range(E.LOOP['n_samples']):
        files = sorted(os.listdir(os.path.join(ck, 'samples', 'sample_%d' % i)))
        assert files == ['model_sample_0.txt', 'model_sample_1.txt'] + ['support_%d.txt' % j for j in range(E.K)]
