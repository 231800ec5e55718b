"""CPU checks of the numpy restatement of a decode state (tests/dstate_ref.py) that the GPU tests compare against -- it continues
gen_ref / filter_ref bitwise, which pins the Philox offset and the window rule without a GPU --, of the binding's struct and its
Python-side shape errors, and of train.train's opt-in sample_condition_on_support key with a fake plugin."""
import ctypes as C
import os

import numpy as np
import pytest

import dstate_ref as D
import filter_ref as F
import gen_ref as R
from conftest import small_config
from oracle import lstm_oracle as O


def _params(cfg, seed=5):
    params = O.glorot_init(cfg, seed)
    params['softmax_b'] = np.random.RandomState(2).randn(*params['softmax_b'].shape) * 2
    return params


CFG = small_config(input_size=30, hidden_size=8, n_layers=2)
PRIMER = np.array([[1, 2, 3, 7], [4, 5, 6, 0]])

# (temperature, top_k, top_p, min_p, theta, window)
SETTINGS = [(1.0, 5, 0.0, 0.0, 1.0, 0), (0.0, 0, 0.0, 0.0, 1.0, 0), (0.8, 6, 0.8, 0.05, 1.5, 5)]


def _one_shot(params, num, T, k, p, m, th, w, primer=PRIMER, seed=7):
    if F.neutral(p, m, th):
        return R.generate(params, CFG, primer.shape[0], num, temperature=T, top_k=k, seed=seed, primer=primer)
    return F.generate(params, CFG, primer.shape[0], num, temperature=T, top_k=k, seed=seed, primer=primer, top_p=p, min_p=m, theta=th,
                      window=w)


@pytest.mark.parametrize('T,k,p,m,th,w', SETTINGS)
def test_e1_feed_primer_then_generate_is_the_one_shot_call(T, k, p, m, th, w):
    params = _params(CFG)
    want_t, want_l = _one_shot(params, 7, T, k, p, m, th, w)
    st = D.State(params, CFG, 2, history=5)           # history = the window: shorter than primer + num
    assert st.feed(PRIMER) is None
    got_t, got_l = st.generate(7, T, k, 7, p, m, th, w)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_l, want_l)
    assert (st.n_ctx, st.n_gen) == (11, 7)


@pytest.mark.parametrize('T,k,p,m,th,w', SETTINGS)
def test_e2_chunked_generate_and_feed(T, k, p, m, th, w):
    params = _params(CFG)
    whole = D.State(params, CFG, 2, history=5)
    whole.feed(PRIMER[:, :1])                          # n_ctx = 1 < window at the start
    want_t, want_l = whole.generate(7, T, k, 3, p, m, th, w)
    parts = D.State(params, CFG, 2, history=5)
    parts.feed(PRIMER[:, :1])
    a_t, a_l = parts.generate(3, T, k, 3, p, m, th, w)
    b_t, b_l = parts.generate(4, T, k, 3, p, m, th, w)
    assert np.array_equal(np.concatenate([a_t, b_t], 1), want_t) and np.array_equal(np.concatenate([a_l, b_l], 1), want_l)
    for x, y in zip(whole.arrays(), parts.arrays()):
        assert np.array_equal(x, y)
    # the second chunk's noise is the one-shot call's at positions 3..6, not 0..3
    again = D.State(params, CFG, 2, history=5)
    again.feed(PRIMER[:, :1])
    again.generate(3, T, k, 3, p, m, th, w)
    again.n_gen = 0
    if T > 0:
        assert not np.array_equal(again.generate(4, T, k, 3, p, m, th, w)[0], b_t)
    # feed in chunks: log-probs and final state
    x = np.random.RandomState(1).randint(0, 31, size=(2, 11))      # the start word (30) may be fed
    one, two = D.State(params, CFG, 2, 6), D.State(params, CFG, 2, 6)
    lp = one.feed(x, logprobs=True)
    lp2 = np.concatenate([two.feed(x[:, :5], logprobs=True), two.feed(x[:, 5:], logprobs=True)], 1)
    assert np.array_equal(lp, lp2)
    for u, v in zip(one.arrays(), two.arrays()):
        assert np.array_equal(u, v)
    assert one.arrays()[2].tolist() == x[:, -6:].tolist() and one.pending == x[:, -1].tolist()


def test_e3_feed_scores_what_generate_reported_and_e4_rows_are_independent():
    params = _params(CFG)
    st = D.State(params, CFG, 3, 40)
    toks, lps = st.generate(9, 1.0, 0, 11)
    again = D.State(params, CFG, 3, 40)
    assert np.array_equal(again.feed(toks, logprobs=True), lps)
    alone = D.State(params, CFG, 1, 40)
    t1, l1 = alone.generate(9, 1.0, 0, 11)
    assert np.array_equal(t1[0], toks[0]) and np.array_equal(l1[0], lps[0])      # row 0 is row 0 whatever the row count


def test_window_rule():
    params = _params(CFG)
    st = D.State(params, CFG, 1, history=6)
    st.feed(np.array([[1, 2]]))
    st.generate(4, 1.0, 0, 1, theta=1.3, window=0)             # n_ctx + num = 6 <= history
    st.reset()
    st.feed(np.array([[1, 2, 3]]))
    with pytest.raises(ValueError):
        st.generate(4, 1.0, 0, 1, theta=1.3, window=0)         # one token too many
    with pytest.raises(ValueError):
        st.generate(1, 1.0, 0, 1, theta=1.3, window=7)         # window > history
    st.generate(4, 1.0, 0, 1, theta=1.3, window=6)
    st.generate(4, 1.0, 0, 1, theta=1.0, window=0)             # no penalty: no rule
    # the whole-context penalty and a window as long as the context agree
    a, b = D.State(params, CFG, 1, 20), D.State(params, CFG, 1, 20)
    for s in (a, b):
        s.feed(np.array([[5, 6, 7]]))
    assert np.array_equal(a.generate(8, 0.9, 0, 2, theta=2.0, window=0)[0], b.generate(8, 0.9, 0, 2, theta=2.0, window=20)[0])


def test_condition_and_eval_conditioned_restatement():
    cfg = small_config(input_size=30, hidden_size=8, max_len=6)
    params = _params(cfg)
    rs = np.random.RandomState(3)
    support, query = rs.randint(0, 30, size=(2, 2, 6)), rs.randint(0, 30, size=(2, 2, 6))
    st = D.condition(params, cfg, support)
    assert st.n_ctx == 2 * 6 + 1 and st.n_gen == 0
    assert st.arrays()[2][0].tolist() == support[0, 0].tolist() + [30] + support[0, 1].tolist()
    # by hand: artist 0, query song 1, as one long row of the fp64 decoder
    inputs = [30] + support[0, 0].tolist() + [30] + support[0, 1].tolist() + [30] + query[0, 1].tolist()
    lg = R.row_logits(params, cfg, inputs[:-1])
    lp = [lg[i][inputs[i + 1]] - R.logsumexp(lg[i]) for i in range(len(inputs) - 1)]
    nll = D.eval_conditioned(params, cfg, support, query)
    rows = D.State(params, cfg, 4, st.history)
    rows.gather(st, [0, 0, 1, 1])
    got = rows.feed(np.concatenate([np.full((4, 1), 30), query.reshape(4, 6)], 1), logprobs=True)
    assert np.allclose(got[1, 1:], lp[-6:], rtol=0, atol=1e-12)
    assert abs(nll + got[:, 1:].mean()) < 1e-12
    # it reads the support set: not the zero-state NLL of the same query songs
    assert abs(nll - O.eval_step(params, query, cfg)) > 1e-3


def test_dstate_config_struct_layout():
    from fsmg.binding import FSMG_DSTATE_CONFIG_VERSION, FsmgDstateConfig
    assert [f[0] for f in FsmgDstateConfig._fields_] == ['version', 'n_rows', 'history', 'reserved']
    assert C.sizeof(FsmgDstateConfig) == 48 and FsmgDstateConfig.reserved.offset == 12 and FsmgDstateConfig.reserved.size == 36
    assert FsmgDstateConfig.n_rows.offset == 4 and FsmgDstateConfig.history.offset == 8
    assert FSMG_DSTATE_CONFIG_VERSION == 1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'fsmg.h')).read()
    assert '#define FSMG_DSTATE_CONFIG_VERSION 1' in header and 'int32_t reserved[9];' in header


class _FakeState(object):
    rows, history, _st = 3, 8, 1


class _FakeEngine(object):
    """an FsmgModel without a library: the shape checks of feed / generate / beam_search run before any call into it"""
    from fsmg.binding import FsmgModel as _M
    feed, generate, beam_search = _M.feed, _M.generate, _M.beam_search


def test_python_side_shape_errors():
    from fsmg.binding import DecodeState
    m, st = _FakeEngine(), _FakeState()
    with pytest.raises(ValueError, match='tokens must be'):
        m.feed(st, np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match='tokens must be'):
        m.feed(st, np.zeros((3, 4, 1), np.int32))
    with pytest.raises(ValueError, match='row count'):
        m.generate(2, 4, state=st)
    with pytest.raises(ValueError, match='no primer'):
        m.generate(3, 4, primer=np.zeros((3, 2), np.int32), state=st)
    with pytest.raises(ValueError, match='row count'):
        m.beam_search(4, 2, n_groups=2, state=st)
    with pytest.raises(ValueError, match='no primer'):
        m.beam_search(4, 2, n_groups=3, primer=np.zeros((3, 2), np.int32), state=st)

    class Cfg(object):
        n_layers, hidden_size = 2, 8
    ds = DecodeState.__new__(DecodeState)
    ds._model, ds.rows, ds.history, ds._st = type('M', (), dict(cfg=Cfg(), _h=None))(), 3, 8, None
    with pytest.raises(ValueError, match='h and c must be'):
        ds.set(np.zeros((2, 3, 7)), np.zeros((2, 3, 8)))
    with pytest.raises(ValueError, match='ctx must be'):
        ds.set(np.zeros((2, 3, 8)), np.zeros((2, 3, 8)), ctx=np.zeros((3, 9), np.int32), n_ctx=20)
    with pytest.raises(ValueError, match='rows must be'):
        ds.gather(ds, [0, 1])
    with pytest.raises(ValueError, match='open DecodeState'):
        ds.gather(None, [0, 1, 2])


class FakeConditionModel(object):
    """a plugin whose generate takes condition_on_support (train.train's opt-in sample_condition_on_support key)"""
    calls = []

    def __init__(self, config):
        FakeConditionModel.calls = []

    def train(self, episode):
        return 1.0

    def eval(self, episode):
        return 1.0

    def save(self, checkpt_path):
        pass

    def recover_or_init(self, init_path):
        pass

    def sample(self, support_set, num):
        FakeConditionModel.calls.append(('sample',))
        return [1] * num

    def generate(self, support_set, num, n=1, temperature=1.0, top_k=0, seed=0, primer_len=0, **kw):
        FakeConditionModel.calls.append(('generate', kw))
        return np.arange(n * num).reshape(n, num) % 5


@pytest.mark.parametrize('keys', ['plain', 'temperature', 'conditioned', 'key_without_temperature'])
def test_train_entry_condition_key(tmp_path, golden_dir, keys):
    import test_train_entry as E
    import train.train as T
    cfg = dict(E.LOOP, name='fake', model_module_name='test_dstate_cpu', model_class_name='FakeConditionModel')
    if keys in ('temperature', 'conditioned'):
        cfg.update(sample_temperature=0.8)
    if keys in ('conditioned', 'key_without_temperature'):
        cfg.update(sample_condition_on_support=True)
    p = E._write_configs(tmp_path, golden_dir, cfg)
    T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', str(tmp_path / 'ck')])
    calls = FakeConditionModel.calls
    if keys in ('plain', 'key_without_temperature'):       # read only inside the sample_temperature branch
        assert calls == [('sample',)] * E.LOOP['n_samples']
    else:
        want = {'condition_on_support': True} if keys == 'conditioned' else {}
        assert calls == [('generate', want)] * E.LOOP['n_samples']
