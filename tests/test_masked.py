"""-m gpu: the padding-masked train / eval passes (include/fsmg.h "per-song lengths").

Two laws carry the file.  Law 1: with every length T a masked call has the unmasked call's bits.  Law 2: the tokens behind a song's
end never matter, exactly.  Then the masked pass against its fp64 restatement (tests/masked_ref.py) with the bounds
tests/test_gpu_parity.py holds the unmasked step to, the eval calls, the indexed and device-resident forms, alternation on one
handle under hipGraph replay, the split form, and the plugin.
"""
import numpy as np
import pytest

import masked_ref as MR
from conftest import small_config
from gpu_utils import f64_params, new_model, rel_max
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

S = ('S', dict(), 2, 2, 1)
S2 = ('S2', dict(n_layers=2), 2, 2, 1)
V12 = ('V12', dict(input_size=12400, hidden_size=16, max_len=6), 2, 2, 1)     # ld > 12288: the three-pass cross entropy
V10 = ('V10', dict(input_size=10000, hidden_size=16, max_len=6), 2, 2, 1)     # k_ce_rows_reg<12>
# the FUSED shape of tests/test_gpu_componentwise.py: the smallest that takes the fused softmax; 2070 rows, not a multiple of 4
F = ('F', dict(input_size=10000, max_len=46, embedding_size=250, hidden_size=512, n_layers=1), 5, 5, 4)

# the paths of the F shape: (environment, whether the pass takes the fused softmax)
PATHS = {
    'default': ({}, True),                               # XCD-partitioned order with the gated projection
    'serial': ({'FSMG_XCD_OVERLAP': '0'}, True),
    'ce_pass': ({'FSMG_FUSED_SOFTMAX': '0'}, False),
    'two_stream': ({'FSMG_OVERLAP': '1'}, False),
    'gemm_f32': ({'FSMG_GEMM': 'f32'}, False),
}


def _case(shape, seed=5):
    """-> cfg, (sup, qry), (support_len, query_len), (sup', qry') with other tokens behind every song's end"""
    name, over, N, K, Q = shape
    cfg = small_config(**over)
    (sup, qry), = O.synthetic_episodes(1, N, K, Q, cfg['max_len'], cfg['input_size'], seed=seed)
    rng = np.random.RandomState(seed + 100)
    ln = MR.lengths_for(rng, (N * (K + Q),), cfg['max_len'])
    sl, ql = ln[:N * K].reshape(N, K), ln[N * K:].reshape(N, Q)
    assert ln.min() == 1 and ln.max() == cfg['max_len'] and len(set(ln.tolist())) > 2
    sup2 = MR.scramble_padding(sup, sl, cfg['input_size'], rng)
    qry2 = MR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) or not np.array_equal(qry, qry2)
    return cfg, (sup.astype(np.int32), qry.astype(np.int32)), (sl, ql), (sup2, qry2)


def _model(shape, monkeypatch, path='default', **kw):
    name, over, N, K, Q = shape
    env, fused = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return new_model(small_config(**over), max_sequences=N * (K + Q), **kw)


def _snapshot(model, run):
    """forward + backward through `run`, then one update: everything the laws compare"""
    run(model)
    out = {'grad:' + k: model.get_grad(k).copy() for k in model.param_shapes}
    out['tail0'] = model.debug_read('tail', 16)[:1].copy()
    out['fused'] = model.debug_read('fused_softmax', 2).copy()
    out['loss'] = np.float32(model.apply_update(1.0))
    for k in model.param_shapes:
        out['param:' + k] = model.get_param(k).copy()
        m, v = model.get_opt_state(k)
        out['m:' + k], out['v:' + k] = m.copy(), v.copy()
    out['step'] = np.int64(model.step)
    return out


def _same(a, b, bitwise_zero_sign=False):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if bitwise_zero_sign:
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k
        else:
            assert np.array_equal(x, y), k


LAW_CASES = [(S, 'default'), (V12, 'default'), (F, 'default'), (F, 'serial'), (F, 'ce_pass')]


@pytest.mark.parametrize('shape,path', LAW_CASES, ids=lambda v: v if isinstance(v, str) else v[0])
def test_full_lengths_are_the_unmasked_step_bit_for_bit(shape, path, monkeypatch):
    cfg, (sup, qry), (sl, ql), _ = _case(shape)
    full_s, full_q = np.full_like(sl, cfg['max_len']), np.full_like(ql, cfg['max_len'])
    a = _snapshot(_model(shape, monkeypatch, path), lambda m: m.forward_backward(sup, qry))
    b = _snapshot(_model(shape, monkeypatch, path), lambda m: m.forward_backward_masked(sup, qry, full_s, full_q))
    if shape is F:
        assert a['fused'][1] == (1.0 if PATHS[path][1] else 0.0) and list(b['fused']) == list(a['fused'])
    _same(a, b, bitwise_zero_sign=True)


@pytest.mark.parametrize('shape,path', LAW_CASES + [(F, 'two_stream'), (F, 'gemm_f32')], ids=lambda v: v if isinstance(v, str) else v[0])
def test_padding_never_matters(shape, path, monkeypatch):
    cfg, (sup, qry), (sl, ql), (sup2, qry2) = _case(shape)
    a = _snapshot(_model(shape, monkeypatch, path), lambda m: m.forward_backward_masked(sup, qry, sl, ql))
    b = _snapshot(_model(shape, monkeypatch, path), lambda m: m.forward_backward_masked(sup2, qry2, sl, ql))
    if shape is F:
        assert a['fused'][1] == (1.0 if PATHS[path][1] else 0.0)
    _same(a, b)
    # ... and the mask is not a no-op: the unmasked step of the same episode differs
    c = _snapshot(_model(shape, monkeypatch, path), lambda m: m.forward_backward(sup, qry))
    assert c['loss'] != a['loss'] and not np.array_equal(c['grad:softmax_w'], a['grad:softmax_w'])


def test_row_weights_and_n_valid(monkeypatch):
    cfg, (sup, qry), (sl, ql), _ = _case(S)
    m = _model(S, monkeypatch)
    m.forward_backward_masked(sup, qry, sl, ql)
    ln = MR.train_lengths(sl, ql)
    T, B = cfg['max_len'], ln.size
    want = np.where(np.arange(T)[:, None] < ln[None, :], np.float32(1.0 / (float(ln.sum()) + 1e-12)), np.float32(0)).astype(np.float32)
    assert np.array_equal(m.debug_read('row_weight', T * B).reshape(T, B), want)
    assert m.debug_read('n_valid', 1)[0] == ln.sum()


_REF = {}


def _reference(shape):
    """the fp64 restatement of one masked step at the handle's seeded parameters: computed once per shape"""
    if shape[0] not in _REF:
        cfg, (sup, qry), (sl, ql), _ = _case(shape)
        name, over, N, K, Q = shape
        model = new_model(cfg, max_sequences=N * (K + Q))
        params = f64_params(model)
        model.close()
        loss, cache, grads, aux = MR.step(params, sup, qry, sl, ql, cfg)
        after = {k: v.copy() for k, v in params.items()}
        O.apply_update(after, grads, aux, O.new_opt_state(after), cfg)
        _REF[shape[0]] = (loss, grads, aux, after)
    return _REF[shape[0]]


@pytest.mark.parametrize('shape', [S, S2, V10, V12, F], ids=lambda v: v[0])
def test_masked_step_against_the_fp64_restatement(shape, monkeypatch):
    """the bounds of tests/test_gpu_parity.py's unmasked step: loss 1e-4, every gradient rel_max < 2e-4, tail[0] 1e-4 relative,
    parameters after one update rel_max < 5e-4"""
    cfg, (sup, qry), (sl, ql), _ = _case(shape)
    loss, grads, aux, after = _reference(shape)
    model = _model(shape, monkeypatch)
    model.forward_backward_masked(sup, qry, sl, ql)
    tail = model.debug_read('tail', 16)
    figures = {'loss': abs(float(tail[1]) - loss), 'tail0': abs(tail[0] - aux['embedding_slices_sq']) / aux['embedding_slices_sq']}
    for name in grads:
        figures['grad:' + name] = rel_max(model.get_grad(name), grads[name])
    got_loss = model.apply_update(1.0)
    for name, ref in after.items():
        figures['param:' + name] = rel_max(model.get_param(name), ref)
    print(shape[0], {k: '%.3g' % v for k, v in figures.items()})
    assert abs(float(got_loss) - loss) <= 1e-4 and figures['loss'] <= 1e-4
    assert figures['tail0'] <= 1e-4
    for k, v in figures.items():
        if k.startswith('grad:'):
            assert v < 2e-4, (k, v)
        if k.startswith('param:'):
            assert v < 5e-4, (k, v)


def test_three_masked_steps_follow_the_oracle(monkeypatch):
    cfg, (sup, qry), (sl, ql), _ = _case(S)
    model = _model(S, monkeypatch)
    params = f64_params(model)
    opt = O.new_opt_state(params)
    for s in range(3):
        want = MR.train_step(params, opt, sup, qry, sl, ql, cfg)
        got = model.train_step_masked(sup, qry, sl, ql)
        assert abs(got - want) <= 1e-4, (s, got, want)
    assert model.step == 3


def test_eval_masked(monkeypatch):
    """three episodes with different n_valid, one of them all length 1"""
    name, over, N, K, Q = S
    cfg = small_config(**over)
    T = cfg['max_len']
    N, Q = 2, 2
    rng = np.random.RandomState(11)
    queries = rng.randint(0, cfg['input_size'], size=(3, N, Q, T)).astype(np.int32)
    lens = np.stack([MR.lengths_for(rng, (N, Q), T), np.ones((N, Q), np.int32), MR.lengths_for(rng, (N, Q), T)])
    lens[2, 0, 0] = T // 2
    assert len({int(l.sum()) for l in lens}) == 3
    model = new_model(cfg)
    params = f64_params(model)
    want = np.array([MR.eval_step(params, queries[e], lens[e], cfg) for e in range(3)])
    got = model.eval_batch_masked(queries, lens)
    assert got.shape == (3,) and np.abs(got - want).max() <= 1e-4, (got, want)
    assert list(model.debug_read('n_valid', 3)) == [float(l.sum()) for l in lens]
    for e in range(3):
        one = model.eval_step_masked(queries[e], lens[e])
        assert abs(one - want[e]) <= 1e-4, (e, one, want[e])
    # full lengths: the unmasked calls' bits
    full = np.full_like(lens, T)
    assert np.array_equal(model.eval_batch_masked(queries, full), model.eval_batch(queries))
    assert np.float32(model.eval_step_masked(queries[0], full[0])) == np.float32(model.eval_step(queries[0]))
    # padding never matters
    other = MR.scramble_padding(queries, lens, cfg['input_size'], rng)
    assert not np.array_equal(other, queries)
    assert np.array_equal(model.eval_batch_masked(other, lens), got)
    # ... and the eval pass leaves the model alone
    for k, v in params.items():
        assert np.array_equal(model.get_param(k), v.astype(np.float32)), k


def test_eval_masked_with_many_one_song_episodes(monkeypatch):
    """12 one-song episodes of max_len 3: twelve groups of one row each, every length of a group its whole n_valid"""
    cfg = small_config(max_len=3)
    rng = np.random.RandomState(12)
    queries = rng.randint(0, cfg['input_size'], size=(12, 1, 1, 3)).astype(np.int32)
    lens = rng.randint(1, 4, size=(12, 1, 1)).astype(np.int32)
    lens[0], lens[1], lens[2] = 1, 2, 3
    model = new_model(cfg)
    params = f64_params(model)
    want = np.array([MR.eval_step(params, queries[e], lens[e], cfg) for e in range(12)])
    got = model.eval_batch_masked(queries, lens)
    assert np.abs(got - want).max() <= 1e-4, (got, want)
    assert list(model.debug_read('n_valid', 12)) == [float(l.sum()) for l in lens]
    w = model.debug_read('row_weight', 36).reshape(3, 12)
    want_w = np.where(np.arange(3)[:, None] < lens.reshape(1, 12), (1.0 / (lens.reshape(1, 12) + 1e-12)).astype(np.float32), np.float32(0))
    assert np.array_equal(w, want_w.astype(np.float32))
    assert np.array_equal(model.eval_batch_masked(queries, np.full_like(lens, 3)), model.eval_batch(queries))


def _table(cfg, n_songs, seed):
    rng = np.random.RandomState(seed)
    table = rng.randint(0, cfg['input_size'], size=(n_songs, cfg['max_len'])).astype(np.int32)
    return table, MR.lengths_for(rng, (n_songs,), cfg['max_len'])


def test_indexed_masked_is_the_masked_step_on_the_gathered_rows(monkeypatch):
    from fsmg.binding import FsmgError
    name, over, N, K, Q = S
    cfg = small_config(**over)
    table, lengths = _table(cfg, 9, 21)
    si, qi = np.array([[0, 8], [3, 3]], np.int32), np.array([[5], [1]], np.int32)
    a, b = new_model(cfg), new_model(cfg)
    b.upload_table(0, table)
    with pytest.raises(FsmgError, match='STATE'):
        b.train_step_indexed_masked(0, si, qi)
    with pytest.raises(FsmgError, match='STATE'):
        b.forward_backward_indexed_masked(0, si, qi)
    b.upload_table(0, table, lengths)
    for s in range(2):
        la = a.train_step_masked(table[si], table[qi], lengths[si], lengths[qi])
        lb = b.train_step_indexed_masked(0, si, qi)
        assert np.float32(la) == np.float32(lb), (s, la, lb)
    for k in a.param_shapes:
        assert np.array_equal(a.get_param(k), b.get_param(k)), k
    a.forward_backward_masked(table[si], table[qi], lengths[si], lengths[qi])
    b.forward_backward_indexed_masked(0, si, qi)
    for k in a.param_shapes:
        assert np.array_equal(a.get_grad(k), b.get_grad(k)), k
    # the table's lengths go when the table is replaced; lengths need a table of the same size
    b.upload_table(0, table)
    with pytest.raises(FsmgError, match='STATE'):
        b.train_step_indexed_masked(0, si, qi)
    with pytest.raises(FsmgError, match='STATE'):
        b._ck(b._lib.fsmg_upload_table_lengths(b._h, 1, lengths.ctypes.data, 9))
    with pytest.raises(FsmgError, match='STATE'):
        b._ck(b._lib.fsmg_upload_table_lengths(b._h, 0, lengths.ctypes.data, 8))
    bad = lengths.copy()
    bad[4] = cfg['max_len'] + 1
    with pytest.raises(FsmgError, match='INVALID'):
        b.upload_table(0, table, bad)


def test_device_resident_tokens_and_lengths(monkeypatch):
    import torch
    from fsmg.binding import FsmgError
    cfg, (sup, qry), (sl, ql), _ = _case(S)
    name, over, N, K, Q = S
    a, b = new_model(cfg), new_model(cfg)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sup, qry, sl, ql)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev]
    for s in range(2):
        la = a.train_step_masked(sup, qry, sl, ql)
        lb = b.train_step_masked(ptr[0], ptr[1], ptr[2], ptr[3], shape=(N, K, Q))
        assert np.float32(la) == np.float32(lb), (s, la, lb)
    for k in a.param_shapes:
        assert np.array_equal(a.get_param(k), b.get_param(k)), k
    assert np.float32(a.eval_step_masked(qry, ql)) == np.float32(b.eval_step_masked(ptr[1], ptr[3], shape=(N, Q)))
    # a device length of 0 or T + 1: the token-range error, parameters and step untouched
    before, step = b.get_params(), b.step
    for wrong in (0, cfg['max_len'] + 1):
        bad = sl.copy()
        bad[1, 0] = wrong
        d_bad = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        with pytest.raises(FsmgError, match='TOKEN_RANGE'):
            b.train_step_masked(ptr[0], ptr[1], d_bad.data_ptr(), ptr[3], shape=(N, K, Q))
        assert b.step == step
        for k, v in before.items():
            assert np.array_equal(b.get_param(k), v), k
        # the same lengths from the host are refused before any device work
        with pytest.raises(FsmgError, match='INVALID'):
            b.train_step_masked(sup, qry, bad, ql)
        with pytest.raises(FsmgError, match='INVALID'):
            b.eval_step_masked(qry, np.full_like(ql, wrong))
    assert b.step == step
    # the handle goes on as if nothing had happened
    assert np.float32(a.train_step_masked(sup, qry, sl, ql)) == np.float32(b.train_step_masked(ptr[0], ptr[1], ptr[2], ptr[3], shape=(N, K, Q)))


def test_masked_and_unmasked_alternate_on_one_handle_under_graph_replay(monkeypatch):
    monkeypatch.setenv('FSMG_EAGER', '0')
    cfg, (sup, qry), (sl, ql), _ = _case(S)

    def grads_of(model, masked):
        if masked:
            model.forward_backward_masked(sup, qry, sl, ql)
        else:
            model.forward_backward(sup, qry)
        out = {k: model.get_grad(k).copy() for k in model.param_shapes}
        out['tail'] = model.debug_read('tail', 2).copy()
        return out

    model = new_model(cfg, use_graph=True)
    first, masked, again, masked_again = grads_of(model, False), grads_of(model, True), grads_of(model, False), grads_of(model, True)
    fresh = grads_of(new_model(cfg, use_graph=True), True)
    _same(first, again)
    _same(masked, fresh)
    _same(masked, masked_again)          # (a replay of the masked graph)
    assert not np.array_equal(first['tail'], masked['tail'])


@pytest.mark.parametrize('shape', [S, F], ids=lambda v: v[0])
def test_forward_backward_masked_plus_apply_update_is_train_step_masked(shape, monkeypatch):
    cfg, (sup, qry), (sl, ql), _ = _case(shape)
    a, b = _model(shape, monkeypatch), _model(shape, monkeypatch)
    a.forward_backward_masked(sup, qry, sl, ql)
    la = a.apply_update(1.0)
    lb = b.train_step_masked(sup, qry, sl, ql)
    assert np.float32(la) == np.float32(lb)
    assert a.step == b.step == 1
    for k in a.param_shapes:
        assert np.array_equal(a.get_param(k), b.get_param(k)), k
        for x, y in zip(a.get_opt_state(k), b.get_opt_state(k)):
            assert np.array_equal(x, y), k


def test_plugin_with_mask_padding(monkeypatch):
    from data.episode import Episode
    from models.lstm_baseline import LSTMBaseline
    cfg, (sup, qry), (sl, ql), _ = _case(S)
    name, over, N, K, Q = S
    plugin = LSTMBaseline(dict(cfg, mask_padding=True))
    plugin.recover_or_init('')
    raw = new_model(cfg)
    raw.set_params(plugin.engine.get_params())
    ep = Episode(sup, qry, support_len=sl, query_len=ql)
    assert np.float32(plugin.eval(ep)) == np.float32(raw.eval_step_masked(qry, ql))
    many = plugin.eval_many([ep, ep])
    assert np.array_equal(np.asarray(many, np.float32), raw.eval_batch_masked(np.stack([qry, qry]), np.stack([ql, ql])))
    assert np.float32(plugin.train(ep)) == np.float32(raw.train_step_masked(sup, qry, sl, ql))
    with pytest.raises(ValueError, match='length'):
        plugin.train(Episode(sup, qry))
    with pytest.raises(ValueError, match='length'):
        plugin.eval(Episode(sup, qry))
