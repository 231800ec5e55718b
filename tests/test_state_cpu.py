"""Batched passes from a carried state (include/fsmg.h fsmg_*_state): everything that needs no GPU.

The fp64 restatement tests/state_ref.py against independent torch autograd (the incoming state detached) and against ONE untruncated
forward over the concatenated segments; the planted mistakes of state_ref.MISTAKES, each of which must move a quantity that
tests/test_gpu_state.py asserts by more than twice that quantity's bound at that file's shapes; the binding's refusals, the header
against the binding, the plugin's keys and segment walk.
"""
import ctypes as C
import os

import numpy as np
import pytest

import maml_ref as MA
import state_ref as S
from conftest import ROOT, small_config
from oracle import lstm_oracle as O

NLL_RTOL, REL_MAX, HS_RTOL = 1e-4, 5e-4, 2e-5          # tests/test_gpu_state.py
# (index into maml_ref.MAML_SHAPES, rows) of tests/test_gpu_state.py CASES
GPU_SHAPES = [(0, 3), (1, 5), (2, 25), (3, 15), (4, 80), (5, 10), (5, 35)]


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def theta_of(cfg):
    return {k: np.asarray(v, np.float64) for k, v in MA.initial_theta(cfg).items()}


# ----------------------------------------------------------------------------- against torch autograd
def torch_segment(params, state, tokens, lengths, cfg):
    """an independent statement in torch: nn.functional only, autograd for every gradient, the incoming state detached"""
    import torch
    import torch.nn.functional as F
    d = O.model_dims(cfg)
    H, L, T, start = d['H'], d['L'], d['T'], d['start']
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    tok = torch.tensor(np.asarray(tokens, np.int64))
    ln = torch.tensor(np.asarray(lengths, np.int64))
    R = tok.shape[0]
    mask = torch.arange(T)[None, :] < ln[:, None]
    x = torch.full((R, T), start, dtype=torch.int64)
    x[:, 1:] = torch.where(mask[:, 1:], tok[:, :-1], torch.tensor(start))
    x[:, 0] = torch.where(ln > 0, torch.tensor(np.asarray(state['pending'], np.int64)), torch.tensor(start))
    y = torch.where(mask, tok, torch.tensor(0))
    inp = F.embedding(x, p['embedding'])
    hs_all, cs_all = [], []
    for l in range(L):
        h = torch.tensor(np.asarray(state['h'][l], np.float64), requires_grad=True).detach()
        c = torch.tensor(np.asarray(state['c'][l], np.float64), requires_grad=True).detach()
        hs, cs, outs = [h], [c], []
        for t in range(T):
            z = torch.cat([inp[:, t], h], dim=1) @ p['kernel_%d' % l] + p['bias_%d' % l]
            i, j, f, o = torch.split(z, H, dim=1)
            c = c * torch.sigmoid(f + O.FORGET_BIAS) + torch.sigmoid(i) * torch.tanh(j)
            h = torch.tanh(c) * torch.sigmoid(o)
            outs.append(h)
            hs.append(h)
            cs.append(c)
        inp = torch.stack(outs, dim=1)
        hs_all.append(torch.stack(hs))
        cs_all.append(torch.stack(cs))
    logits = inp.reshape(R * T, H) @ p['softmax_w'] + p['softmax_b']
    nll = F.cross_entropy(logits, y.reshape(-1), reduction='none').reshape(R, T)
    loss = (nll * mask).sum() / (float(ln.sum()) + 1e-12)
    loss.backward()
    rows = torch.arange(R)
    h1 = torch.stack([torch.where((ln > 0)[:, None], hs_all[l][ln, rows], hs_all[l][0]) for l in range(L)])
    c1 = torch.stack([torch.where((ln > 0)[:, None], cs_all[l][ln, rows], cs_all[l][0]) for l in range(L)])
    return dict(loss=float(loss.detach()), logprob=(-nll * mask).detach().numpy(), grads={k: v.grad.numpy() for k, v in p.items()},
                h=h1.detach().numpy(), c=c1.detach().numpy())


@pytest.mark.parametrize('over', [dict(hidden_size=20, embedding_size=10, input_size=50, max_len=7),
                                  dict(hidden_size=12, embedding_size=6, input_size=30, max_len=5, n_layers=2)], ids=['one-layer', 'two-layers'])
def test_restatement_equals_torch_autograd_with_the_state_detached(over):
    cfg = small_config(**over)
    R, T = 6, cfg['max_len']
    theta = theta_of(cfg)
    seg = S.segments(cfg, R, 3, 3)
    lens = [None, S.ragged_lengths(np.random.RandomState(1), R, T), S.ragged_lengths(np.random.RandomState(2), R, T)[::-1].copy()]
    st = S.fresh_state(cfg, R)
    for tok, ln in zip(seg, lens):
        want = torch_segment(theta, st, tok, np.full(R, T) if ln is None else ln, cfg)
        got, st = S.segment(theta, st, tok, ln, cfg)
        assert abs(got['loss'] - want['loss']) <= 1e-9 * abs(want['loss'])
        assert np.abs(got['logprob'] - want['logprob']).max() <= 1e-9
        for k in want['grads']:
            assert rel_max(got['grads'][k], want['grads'][k]) <= 1e-9, k
        assert np.abs(st['h'] - want['h']).max() <= 1e-9 and np.abs(st['c'] - want['c']).max() <= 1e-9


def test_three_segments_equal_one_untruncated_forward_and_differ_in_the_gradient():
    cfg = small_config(hidden_size=20, embedding_size=10, input_size=50, max_len=6)
    R, T = 4, cfg['max_len']
    theta = theta_of(cfg)
    seg = S.segments(cfg, R, 3, 4)
    st = S.fresh_state(cfg, R)
    lps, grads = [], []
    for tok in seg:
        r, st = S.segment(theta, st, tok, None, cfg)
        lps.append(r['logprob'])
        grads.append(r['grads'])
    # ONE forward over 3 T tokens from the zero state
    long_cfg = dict(cfg, max_len=3 * T)
    songs = np.concatenate(seg, axis=1)
    X, Y, mask = S.device_xy(songs, np.full(R, 3 * T), np.full(R, cfg['input_size']), cfg['input_size'])
    W = np.zeros((R, 3 * T))
    W[:, 2 * T:] = 1.0 / (R * T + 1e-12)                 # the third segment's loss alone
    z = S.fresh_state(cfg, R)
    full = S.run(theta, z['h'], z['c'], X, Y, W, long_cfg)
    assert np.abs(np.concatenate(lps, axis=1) - full['logprob']).max() <= 1e-12
    assert np.abs(st['h'] - full['hs'][:, -1]).max() <= 1e-12 and np.abs(st['c'] - full['cs'][:, -1]).max() <= 1e-12
    # ... whose gradient flows through the first two segments: not the truncated one
    for k in ('kernel_0', 'embedding'):
        assert rel_max(grads[2][k], full['grads'][k]) > 1e-3, k
    assert rel_max(grads[2]['softmax_w'], full['grads']['softmax_w']) <= 1e-12        # (the projection sees the same states)
    # the context rule over the three segments
    assert np.array_equal(st['ctx'], songs) and np.array_equal(st['pending'], songs[:, -1])


# ----------------------------------------------------------------------------- the planted mistakes
def asserted_ratios(got, got_state, ref64, st64, ref32, st32):
    """every quantity tests/test_gpu_state.py asserts on a segment, as deviation / bound"""
    out = {}
    e32 = np.abs(ref32['logprob'].astype(np.float64) - ref64['logprob']).max()
    out['logprob'] = float((np.abs(got['logprob'] - ref64['logprob']) / np.maximum(NLL_RTOL * np.abs(ref64['logprob']), 8 * e32 + 1e-300)).max())
    out['loss'] = abs(float(got['loss']) - float(ref64['loss'])) / (NLL_RTOL * abs(float(ref64['loss'])))
    for k in ref64['grads']:
        out[k] = rel_max(got['grads'][k], ref64['grads'][k]) / max(REL_MAX, 8 * rel_max(ref32['grads'][k], ref64['grads'][k]))
    for part in ('h', 'c'):
        out['state ' + part] = rel_max(got_state[part], st64[part]) / max(HS_RTOL, 8 * rel_max(st32[part], st64[part]))
    return out


WHERE = dict(start_word=('logprob',), no_c=('logprob', 'state c'), no_hprev_dk=('kernel_0',), export_T=('state h', 'state c'),
             swap_layers=('logprob',), table_start=('embedding',), grad_through_state=('kernel_0', 'embedding'))


@pytest.mark.parametrize('shape', GPU_SHAPES, ids=lambda s: 'shape%d-%drows' % s)
def test_every_planted_mistake_moves_an_asserted_quantity_by_twice_its_bound(shape):
    idx, rows = shape
    cfg = MA.config_of(MA.MAML_SHAPES[idx], max_grad_norm=5)
    T = cfg['max_len']
    theta = theta_of(cfg)
    seg = S.segments(cfg, rows, 2, 21)
    ln = S.ragged_lengths(np.random.RandomState(7), rows, T)
    s0 = S.fresh_state(cfg, rows)
    _, s1 = S.segment(theta, s0, seg[0], None, cfg, want_grads=False)
    ref64, st64 = S.segment(theta, s1, seg[1], ln, cfg)
    _, s1_32 = S.segment(theta, S.fresh_state(cfg, rows, np.float32), seg[0], None, cfg, dtype=np.float32, want_grads=False)
    ref32, st32 = S.segment(theta, s1_32, seg[1], ln, cfg, dtype=np.float32)
    clean = asserted_ratios(ref32, st32, ref64, st64, ref32, st32)
    assert max(clean.values()) <= 1.0, clean                # the fp32 restatement itself is inside every bound
    for mistake in S.MISTAKES:
        if mistake == 'swap_layers' and cfg['n_layers'] < 2:
            continue
        got, st = S.segment(theta, s1, seg[1], ln, cfg, mistake=mistake, prev=(s0, seg[0], np.full(rows, T)))
        ratios = asserted_ratios(got, st, ref64, st64, ref32, st32)
        moved = max(ratios[k] for k in WHERE[mistake])
        print('STATE|planted|shape %d rows %d|%s|%.3g x bound' % (idx, rows, mistake, moved))
        assert moved > 2.0, (mistake, ratios)


# ----------------------------------------------------------------------------- the binding
def test_state_config_struct_layout_and_symbols():
    from fsmg.binding import FSMG_STATE_CONFIG_VERSION, FSMG_STATE_PASS_ROWS, SIGNATURES, FsmgStateConfig
    assert [f[0] for f in FsmgStateConfig._fields_] == ['version', 'tokens_on_device', 'reserved']
    assert C.sizeof(FsmgStateConfig) == 32 and FsmgStateConfig.tokens_on_device.offset == 4 and FsmgStateConfig.reserved.offset == 8
    header = open(os.path.join(ROOT, 'include', 'fsmg.h')).read()
    assert '#define FSMG_STATE_CONFIG_VERSION %d' % FSMG_STATE_CONFIG_VERSION in header
    assert '#define FSMG_STATE_PASS_ROWS %d' % FSMG_STATE_PASS_ROWS in header
    assert 'int32_t reserved[6];' in header
    for name, nargs in (('fsmg_score_state', 10), ('fsmg_eval_step_state', 7), ('fsmg_forward_backward_state', 5), ('fsmg_train_step_state', 6)):
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == nargs, name
        decl = header[header.index('int %s(' % name):]
        assert decl[:decl.index(';')].count(',') + 1 == nargs, name


class _FakeEngine(object):
    """an FsmgModel without a library: the checks of the state calls run before any call into it"""
    from fsmg.binding import FsmgModel as _M
    max_len = 6
    _lib = type('Lib', (), dict(fsmg_score_state=None, fsmg_eval_step_state=None, fsmg_forward_backward_state=None, fsmg_train_step_state=None))()
    _state_args, score_state, eval_step_state = _M._state_args, _M.score_state, _M.eval_step_state
    forward_backward_state, train_step_state = _M.forward_backward_state, _M.train_step_state


def test_python_side_refusals():
    from fsmg.binding import DecodeState
    m = _FakeEngine()
    st = DecodeState.__new__(DecodeState)
    st._model, st.rows, st.history, st._st = m, 3, 4, None
    other = DecodeState.__new__(DecodeState)
    other._model, other.rows, other.history, other._st = _FakeEngine(), 3, 4, None
    ok = np.zeros((3, 6), np.int32)
    for call in (m.score_state, m.eval_step_state, m.forward_backward_state, m.train_step_state):
        with pytest.raises(ValueError, match='DecodeState of this model'):
            call(other, ok)
        with pytest.raises(ValueError, match='DecodeState of this model'):
            call(None, ok)
        with pytest.raises(ValueError, match='tokens must be'):
            call(st, np.zeros((3, 5), np.int32))
        with pytest.raises(ValueError, match='tokens must be'):
            call(st, np.zeros((2, 6), np.int32))
        with pytest.raises(ValueError, match='lengths for'):
            call(st, ok, lengths=[1, 2])
        with pytest.raises(Exception, match='closed'):           # everything checked: the call reaches the (closed) state
            call(st, ok, lengths=[1, 2, 0])


# ----------------------------------------------------------------------------- the plugin
def test_plugin_keys_config_and_segment_walk():
    import yaml
    from models import tbptt_lstm as P
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'lstm_tbptt.yaml')))
    assert cfg['model_module_name'] == 'models.tbptt_lstm' and cfg['model_class_name'] == 'TBPTTLSTM'
    assert cfg['segment_len'] == 32 and cfg['mask_padding'] is True
    assert issubclass(P.TBPTTLSTM, __import__('models.lstm_baseline', fromlist=['LSTMBaseline']).LSTMBaseline)
    with pytest.raises(RuntimeError, match='segment_len'):
        P.TBPTTLSTM(small_config())
    with pytest.raises(RuntimeError, match='segment_len must be'):
        P.TBPTTLSTM(small_config(segment_len=11))
    # train.train finds no index fast path
    assert not hasattr(P.TBPTTLSTM.__new__(P.TBPTTLSTM), 'train_indexed') and not hasattr(P.TBPTTLSTM.__new__(P.TBPTTLSTM), 'attach_table')
    # the walk: ceil(max_len / segment_len) segments, the last ragged, none behind the longest song
    plan = P.segment_plan(10, [10, 7, 4, 1], 4)
    assert [s0 for s0, _ in plan] == [0, 4, 8]
    assert [ln.tolist() for _, ln in plan] == [[4, 4, 4, 1], [4, 3, 0, 0], [2, 0, 0, 0]]
    assert [s0 for s0, _ in P.segment_plan(10, [5, 3], 4)] == [0, 4]
    assert sum(int(ln.sum()) for _, ln in plan) == 22
    songs = np.arange(20, dtype=np.int32).reshape(2, 10)
    assert np.array_equal(P.segment_tokens(songs, 8, 4), [[8, 9, 0, 0], [18, 19, 0, 0]])
    assert np.array_equal(P.segment_tokens(songs, 4, 4), songs[:, 4:8])
    # the walk in the restatement: segments' NLL numerators over the total n_valid = the full-length masked NLL
    mcfg = small_config(hidden_size=12, embedding_size=6, input_size=30, max_len=4)
    theta = theta_of(mcfg)
    rng = np.random.RandomState(0)
    full = rng.randint(0, 30, size=(4, 10)).astype(np.int32)
    lengths = np.array([10, 7, 4, 1])
    st, num = S.fresh_state(mcfg, 4), 0.0
    for s0, ln in plan:
        r, st = S.segment(theta, st, P.segment_tokens(full, s0, 4), ln, mcfg, want_grads=False)
        num += float(r['loss']) * int(ln.sum())
    long_cfg = dict(mcfg, max_len=10)
    X, Y, mask = S.device_xy(full, lengths, np.full(4, 30), 30)
    z = S.fresh_state(mcfg, 4)
    want = S.run(theta, z['h'], z['c'], X, Y, mask / (22 + 1e-12), long_cfg, want_grads=False)['loss']
    assert abs(num / 22 - want) <= 1e-12 * abs(want)
