"""The MAML-style step with per-song lengths without a GPU: the fp64 restatement (tests/maml_masked_ref.py) against
the oracle at full lengths, its padding law, an independent torch-autograd statement of the same objective, four planted mistakes
that each fail those checks, and the way of `maml_lengths` from the plugin through fsmg.dist.EpisodeParallel and the engine to the
masked calls of the binding -- with recorders in the place of the library."""
import os

import numpy as np
import pytest
import yaml

import maml_masked_ref as MM
import maml_ref as MR
import masked_ref as KR
from conftest import ROOT, small_config
from oracle import lstm_oracle as O

LR = MR.INNER_LR
CPU_SHAPES = [MR.MAML_SHAPES[0], MR.MAML_SHAPES[1]]          # one row per set; stacked layers with two inner steps


def setup(shape, **over):
    cfg = MR.config_of(shape, **over)
    sup, qry = MR.episode(cfg, shape)
    sl, ql = MM.lengths_of(shape, cfg['max_len'])
    return cfg, sup, qry, sl, ql, MR.f64(MR.initial_theta(cfg))


def same64(a, b):
    return all(np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)) for k in a) and a.keys() == b.keys()


# ----------------------------------------------------------------------------- the restatement and the oracle
@pytest.mark.parametrize('mode', ['tf1_slices', 'dense'])
@pytest.mark.parametrize('shape', CPU_SHAPES, ids=MR.shape_id)
def test_full_lengths_are_the_oracle_bit_for_bit(shape, mode):
    cfg, sup, qry, sl, ql, p64 = setup(shape)
    n, T = shape[4], cfg['max_len']
    fs, fq = np.full_like(sl, T), np.full_like(ql, T)
    r = MM.query_grads(p64, sup, qry, fs, fq, cfg, n, LR, mode)
    fast, losses = O.maml_adapt(p64, sup, cfg, n, LR, clip_norm_mode=mode)
    loss, grads, aux = O.maml_query_grads(p64, sup, qry, cfg, n, LR, clip_norm_mode=mode)
    assert same64(r['theta'], fast) and [s['loss'] for s in r['steps']] == losses
    assert r['loss'] == loss and r['aux'] == aux and same64(r['grads'], grads)
    assert MM.maml_eval(p64, sup, qry, fs, fq, cfg, n, LR, mode) == O.maml_eval(p64, sup, qry, cfg, n, LR, clip_norm_mode=mode)
    a, b = {k: v.copy() for k, v in p64.items()}, {k: v.copy() for k, v in p64.items()}
    oa, ob = O.new_opt_state(a), O.new_opt_state(b)
    for _ in range(2):
        assert MM.maml_step(a, oa, sup, qry, fs, fq, cfg, n, LR, mode) == O.maml_step(b, ob, sup, qry, cfg, n, LR, clip_norm_mode=mode)
    assert same64(a, b) and same64(oa['m'], ob['m']) and same64(oa['v'], ob['v']) and oa['step'] == ob['step'] == 2
    # ... and shorter songs are another computation
    assert MM.query_grads(p64, sup, qry, sl, ql, cfg, n, LR, mode)['loss'] != loss


# ----------------------------------------------------------------------------- the two checks every variant is put through
def _torch_pass(p, tokens, lengths, cfg):
    """torch autograd, fp64: the masked mean cross entropy of `tokens` [.., T] as the caller gave them (nothing replaced behind a
    song's end) at the tensors p -> (loss, {name: gradient}, squared norm of the embedding slices' gradient)"""
    import torch
    import torch.nn.functional as F
    d = O.model_dims(cfg)
    H, L, T = d['H'], d['L'], d['T']
    X, Y = O.tokens_to_input_and_target(tokens, d['start'])
    p = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    x = p['embedding'][torch.tensor(X, dtype=torch.long)]
    x.retain_grad()
    slices = x
    B = x.shape[0]
    for l in range(L):
        K, b = p['kernel_%d' % l], p['bias_%d' % l]
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        outs = []
        for t in range(T):
            i, j, f, o = (torch.cat([x[:, t], h], dim=1) @ K + b).split(H, dim=1)
            c = c * torch.sigmoid(f + O.FORGET_BIAS) + torch.sigmoid(i) * torch.tanh(j)
            h = torch.tanh(c) * torch.sigmoid(o)
            outs.append(h)
        x = torch.stack(outs, dim=1)
    logits = x.reshape(B * T, H) @ p['softmax_w'] + p['softmax_b']
    ce = F.cross_entropy(logits, torch.tensor(Y.reshape(-1), dtype=torch.long), reduction='none')
    lengths = np.asarray(lengths).reshape(-1)
    mask = torch.tensor((np.arange(T)[None, :] < lengths[:, None]).reshape(-1))
    loss = ce[mask].sum() / (float(lengths.sum()) + 1e-12)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in p.items()}, float((slices.grad ** 2).sum())


def torch_maml(params, sup, qry, sl, ql, cfg, n, lr, mode):
    """the objective of DESIGN.md 22 stated with autograd: clipped SGD on the masked support loss, first order, then the masked query
    loss at theta' and its gradient -> dict(theta, loss, grads) in numpy"""
    import torch
    fast = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    clip = float(cfg['max_grad_norm'])
    for _ in range(n):
        _, g, slices_sq = _torch_pass(fast, sup, sl, cfg)
        sq = sum(float((g[k] ** 2).sum()) for k in g if not (k == 'embedding' and mode == 'tf1_slices'))
        gnorm = np.sqrt(sq + (slices_sq if mode == 'tf1_slices' else 0.0))
        fast = {k: fast[k] - lr * (g[k] * (clip / max(gnorm, clip))) for k in fast}
    loss, g, _ = _torch_pass(fast, qry, ql, cfg)
    return dict(theta={k: v.numpy() for k, v in fast.items()}, loss=float(loss), grads={k: v.numpy() for k, v in g.items()})


def failures_of(compute, shape, mode='tf1_slices', **over):
    """`compute(params, sup, qry, sl, ql, cfg, n, lr, mode)` -> dict(theta, loss, grads) through the two checks:
      A  agreement with torch_maml to 1e-9 (the bound the MAML oracle is held to against autograd) -- theta', L_qry, outer gradients;
      P  other in-range ids behind every song's end change nothing, exactly.
    -> list of strings, empty when both hold"""
    cfg, sup, qry, sl, ql, p64 = setup(shape, **over)
    n = shape[4]
    assert int(sl.sum()) != int(ql.sum())
    got = compute(p64, sup, qry, sl, ql, cfg, n, LR, mode)
    want = torch_maml(p64, sup, qry, sl, ql, cfg, n, LR, mode)
    out = []
    if not abs(got['loss'] - want['loss']) <= 1e-9:
        out.append('A loss %.12g, autograd %.12g' % (got['loss'], want['loss']))
    for what in ('theta', 'grads'):
        for k in sorted(want[what]):
            err = np.abs(got[what][k] - want[what][k]).max()
            if not err <= 1e-9 * max(1.0, np.abs(want[what][k]).max()):
                out.append('A %s %s off by %.3g' % (what, k, err))
    rng = np.random.RandomState(77)
    sup2, qry2 = KR.scramble_padding(sup, sl, cfg['input_size'], rng), KR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) and not np.array_equal(qry, qry2)
    again = compute(p64, sup2, qry2, sl, ql, cfg, n, LR, mode)
    if again['loss'] != got['loss']:
        out.append('P loss moved with the padding')
    out += ['P %s %s moved with the padding' % (what, k) for what in ('theta', 'grads') for k in sorted(got[what])
            if not np.array_equal(again[what][k], got[what][k])]
    return out


def restatement(wrong=None):
    return lambda p, sup, qry, sl, ql, cfg, n, lr, mode: MM.query_grads(p, sup, qry, sl, ql, cfg, n, lr, mode, wrong=wrong)


@pytest.mark.parametrize('mode,max_grad_norm', [('tf1_slices', MR.MAX_GRAD_NORM), ('dense', MR.MAX_GRAD_NORM),
                                                ('tf1_slices', MR.MAX_GRAD_NORM_INACTIVE)])
@pytest.mark.parametrize('shape', CPU_SHAPES, ids=MR.shape_id)
def test_restatement_agrees_with_autograd_and_ignores_the_padding(shape, mode, max_grad_norm):
    assert failures_of(restatement(), shape, mode, max_grad_norm=max_grad_norm) == []


@pytest.mark.parametrize('wrong', MM.WRONG)
def test_a_planted_mistake_fails_the_checks(wrong):
    """every one of them is shown failing, under the active and under the inactive clip (an active clip divides a wrong
    normalisation out of theta' -- the loss and the outer gradients still carry it)"""
    shape = MR.MAML_SHAPES[1]                   # two inner steps: `lengths_dropped_on_step_2` has a second step to drop them on
    for max_grad_norm in (MR.MAX_GRAD_NORM, MR.MAX_GRAD_NORM_INACTIVE):
        bad = failures_of(restatement(wrong), shape, max_grad_norm=max_grad_norm)
        print('TEETH|%s|%s|%s' % (wrong, max_grad_norm, bad[:4]))
        assert bad, (wrong, max_grad_norm)
        kinds = {b[0] for b in bad}
        if wrong == 'padding_ids_in_embedding_grad':
            assert 'P' in kinds and any('embedding' in b for b in bad)
        elif wrong == 'rows_times_T':
            assert kinds == {'A'}, bad              # a wrong denominator still ignores the padding
        else:
            assert 'A' in kinds, bad                # (wrong lengths read ids the right ones call padding: P may fail as well)
        if wrong in ('query_lengths_on_support', 'lengths_dropped_on_step_2'):
            assert any(b.startswith('A theta') for b in bad)
    cfg, sup, qry, sl, ql, p64 = setup(shape)
    want = MM.maml_eval(p64, sup, qry, sl, ql, cfg, shape[4], LR)
    assert want == MM.query_grads(p64, sup, qry, sl, ql, cfg, shape[4], LR)['loss']
    if wrong != 'padding_ids_in_embedding_grad':    # (the NLL of an evaluation has no embedding gradient in it)
        assert MM.maml_eval(p64, sup, qry, sl, ql, cfg, shape[4], LR, wrong=wrong) != want


# ----------------------------------------------------------------------------- plumbing: the key's way to the masked calls
class Engine(object):
    """what fsmg.dist.EpisodeParallel drives, recording"""
    def __init__(self, fused, library_comm=False):
        self.calls, self.library_comm = [], library_comm
        if fused:
            self.fused_maml_step = self._fused

    def _fused(self, support, query, inner_steps, inner_lr, want_loss=True, table=None, **kw):
        self.calls.append(('fused', table, kw))
        return 1.0

    def maml_forward_backward(self, support, query, inner_steps, inner_lr, **kw):
        self.calls.append(('fb', kw))

    def maml_forward_backward_indexed(self, table, support, query, inner_steps, inner_lr, **kw):
        self.calls.append(('fbi', table, kw))

    def apply_update(self, scale, want_loss=True):
        return 2.0


def test_episode_parallel_routes_maml_lengths_on_all_three_paths():
    from fsmg.dist import EpisodeParallel
    lens = (np.ones((1, 1), np.int32), np.ones((1, 1), np.int32))
    maml = (1, 0.1)
    e = Engine(fused=True)
    p = EpisodeParallel(e)
    p.train_step('s', 'q', maml=maml)                                   # split: one process has nothing to fuse the token form with
    p.train_step('s', 'q', maml=maml, table=0)
    p.train_step('s', 'q', maml=maml, maml_lengths=lens)
    p.train_step('s', 'q', maml=maml, table=0, maml_lengths=True)
    assert e.calls == [('fb', {}), ('fused', 0, {}), ('fb', {'maml_lengths': lens}), ('fused', 0, {'maml_lengths': True})]
    e = Engine(fused=False)
    p = EpisodeParallel(e)
    p.train_step('s', 'q', maml=maml, table=0)
    p.train_step('s', 'q', maml=maml, table=0, maml_lengths=True)
    assert e.calls == [('fbi', 0, {}), ('fbi', 0, {'maml_lengths': True})]
    e = Engine(fused=True, library_comm=True)                              # the library owns the exchange: one fused call per step
    p = EpisodeParallel(e)
    p.train_step('s', 'q', maml=maml)
    p.train_step('s', 'q', maml=maml, maml_lengths=lens)
    assert e.calls == [('fused', None, {}), ('fused', None, {'maml_lengths': lens})]
    # the keyword goes with maml= only, and its two forms go with tokens / a table
    with pytest.raises(ValueError, match='maml='):
        p.train_step('s', 'q', maml_lengths=lens)
    with pytest.raises(ValueError, match='table'):
        p.train_step('s', 'q', maml=maml, maml_lengths=True)
    with pytest.raises(ValueError, match='table'):
        p.train_step('s', 'q', maml=maml, table=0, maml_lengths=lens)
    # the pinned refusal of tests/test_masked_cpu.py: `lengths` is the plain step's keyword
    with pytest.raises(ValueError, match='MAML'):
        p.train_step('s', 'q', lengths=lens, maml=maml)


class Binding(object):
    """FsmgModel's MAML methods, recording (name, positional arguments, keywords)"""
    max_len = 4

    def __init__(self):
        self.calls = []

    def apply_update(self, grad_scale=1.0, want_loss=True):       # (the split route's second half: not recorded)
        return 1.5

    def __getattr__(self, name):
        if not (name.startswith('maml_') or name == 'upload_table'):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append((name, a, kw))
            return 1.5
        return call


def plugin_with_recorder(maml_lengths):
    from fsmg.dist import EpisodeParallel
    from models.maml_lstm import MAMLLSTM
    m = MAMLLSTM.__new__(MAMLLSTM)          # no device: the members the MAML methods read, by hand
    m._model, m._initialised, m._scalars = Binding(), True, None
    m._inner_steps, m._inner_lr, m.maml_lengths, m.mask_padding = 2, 0.25, maml_lengths, False
    m._train_calls = m._eval_calls = 0
    m._parallel = EpisodeParallel(m)
    return m


def _episode(lengths=True):
    from data.episode import Episode
    rng = np.random.RandomState(1)
    sup, qry = rng.randint(0, 9, size=(2, 3, 4)).astype(np.int32), rng.randint(0, 9, size=(2, 1, 4)).astype(np.int32)
    sl, ql = np.array([[1, 4, 2], [3, 4, 1]], np.int32), np.array([[4], [2]], np.int32)
    return (Episode(sup, qry, sl, ql) if lengths else Episode(sup, qry)), sup, qry, sl, ql


def test_plugin_hands_the_lengths_to_the_masked_calls():
    ep, sup, qry, sl, ql = _episode()
    m = plugin_with_recorder(True)
    b = m._model
    assert m.train(ep) == 1.5 and m.eval(ep) == 1.5
    m.attach_table('train', np.zeros((5, 4), np.int32), np.arange(1, 6, dtype=np.int32) % 4 + 1)
    m.train_indexed('train', np.zeros((2, 3), np.int32), np.zeros((2, 1), np.int32), want_loss=True)
    flat, flat_len = sup.reshape(6, 4), sl.reshape(6)
    m.generate(flat, 3, n=2, support_len=flat_len)
    m.beam_search(flat, 3, 2, support_len=flat_len)
    m.score(flat, qry.reshape(2, 4), support_len=flat_len, lengths=ql.reshape(2))
    names = [c[0] for c in b.calls]
    assert names == ['maml_forward_backward_masked', 'maml_eval_masked', 'upload_table', 'maml_step_indexed_masked', 'maml_generate',
                     'maml_beam_search', 'maml_score']
    fb, ev, up, idx, gen, beam, score = b.calls
    for call in (fb, ev):
        assert np.array_equal(call[1][0], sup) and np.array_equal(call[1][1], qry)
        assert np.array_equal(call[1][2], sl) and np.array_equal(call[1][3], ql) and call[1][4:] == (2, 0.25)
    assert up[1][0] == 0 and up[1][2] is not None and len(up[1][2]) == 5
    assert idx[1][0] == 0 and idx[1][3:] == (2, 0.25)
    for call in (gen, beam, score):
        assert np.array_equal(call[2]['support_len'], flat_len)
    assert np.array_equal(score[2]['lengths'], ql.reshape(2))
    # a missing length is a ValueError, wherever it is missing
    bare = _episode(lengths=False)[0]
    for call in (lambda: m.train(bare), lambda: m.eval(bare), lambda: m.generate(flat, 3), lambda: m.beam_search(flat, 3, 2),
                 lambda: m.score(flat, qry.reshape(2, 4)), lambda: m.attach_table('train', np.zeros((5, 4), np.int32)),
                 lambda: m.generate(flat, 3, support_len=flat_len[:5])):
        with pytest.raises(ValueError, match='length|support_len'):
            call()
    assert [c[0] for c in b.calls] == names             # ... raised before anything reached the library


def test_without_the_key_nothing_new_is_passed():
    ep, sup, qry, sl, ql = _episode()
    m = plugin_with_recorder(False)
    b = m._model
    m.train(ep)
    m.eval(ep)
    m.attach_table('train', np.zeros((5, 4), np.int32), np.ones(5, np.int32))       # lengths offered, not wanted: not uploaded
    m.train_indexed('train', np.zeros((2, 3), np.int32), np.zeros((2, 1), np.int32), want_loss=True)
    flat = sup.reshape(6, 4)
    m.generate(flat, 3, n=2)
    m.beam_search(flat, 3, 2)
    m.score(flat, qry.reshape(2, 4))
    assert [c[0] for c in b.calls] == ['maml_forward_backward', 'maml_eval', 'upload_table', 'maml_step_indexed', 'maml_generate',
                                       'maml_beam_search', 'maml_score']
    assert b.calls[0][1][2:] == (2, 0.25) and b.calls[0][2] == {} and b.calls[1][1][2:] == (2, 0.25) and b.calls[1][2] == {}
    assert b.calls[2][1][2] is None
    for call in b.calls[4:]:
        assert 'support_len' not in call[2] and 'lengths' not in call[2]
    with pytest.raises(ValueError, match='maml_lengths'):
        m.generate(flat, 3, support_len=sl.reshape(6))


def test_the_binding_keeps_the_old_calls_and_knows_the_new_ones():
    """absent keywords mean the old call, argument for argument: FsmgModel's decode methods with a recording library"""
    from fsmg import binding as B
    for name in ('fsmg_maml_forward_backward_masked', 'fsmg_maml_step_masked', 'fsmg_maml_eval_masked',
                 'fsmg_maml_forward_backward_indexed_masked', 'fsmg_maml_step_indexed_masked', 'fsmg_maml_generate_filtered_masked',
                 'fsmg_maml_beam_search_masked', 'fsmg_maml_score_masked'):
        twin = name.replace('_masked', '')
        extra = {'fsmg_maml_score_masked': 2}.get(name, 0 if 'indexed' in name else 2 if 'filtered' not in name and 'beam' not in name else 1)
        assert len(B.SIGNATURES[name][1]) == len(B.SIGNATURES[twin][1]) + extra, name

    class Lib(object):
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def fn(*a):
                self.calls.append((name, len(a)))
                return 0
            return fn
    m = B.FsmgModel.__new__(B.FsmgModel)
    m._lib, m._h, m.max_len = Lib(), None, 4
    m._ck = lambda rc: None
    sup, ln = np.zeros((3, 4), np.int32), np.array([1, 4, 2], np.int32)
    m.maml_generate(sup, 2, 1, 0.1)
    m.maml_generate(sup, 2, 1, 0.1, top_p=0.5)
    m.maml_generate(sup, 2, 1, 0.1, support_len=ln)
    m.maml_beam_search(sup, 2, 1, 0.1, 2)
    m.maml_beam_search(sup, 2, 1, 0.1, 2, support_len=ln)
    m.maml_score(sup, sup, 1, 0.1)
    m.maml_score(sup, sup, 1, 0.1, support_len=ln)
    m.maml_score(sup, sup, 1, 0.1, support_len=ln, lengths=ln)
    sig = lambda n: len(B.SIGNATURES[n][1])
    assert m._lib.calls == [(n, sig(n)) for n in ('fsmg_maml_generate', 'fsmg_maml_generate_filtered', 'fsmg_maml_generate_filtered_masked',
                                                   'fsmg_maml_beam_search', 'fsmg_maml_beam_search_masked', 'fsmg_maml_score',
                                                   'fsmg_maml_score_masked', 'fsmg_maml_score_masked')]
    with pytest.raises(ValueError):
        m.maml_generate(sup, 2, 1, 0.1, support_len=ln[:2])           # two lengths for three support songs
    with pytest.raises(ValueError, match='support_len'):
        m.maml_score(sup, sup, 1, 0.1, lengths=ln)
    with pytest.raises(ValueError, match=r'\[1, 4\]'):
        m.maml_score(sup, sup, 1, 0.1, support_len=ln, lengths=np.array([1, 5, 2]))


def test_the_pinned_refusal_and_the_config():
    from models.maml_lstm import MAMLLSTM
    with pytest.raises(RuntimeError, match='MAMLLSTM has no padding-masked loss'):
        MAMLLSTM(dict(small_config(), mask_padding=True))
    assert MAMLLSTM.MASKS_PADDING is False
    conf = os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config')
    masked = yaml.safe_load(open(os.path.join(conf, 'maml_masked_lstm.yaml')))
    base = yaml.safe_load(open(os.path.join(conf, 'maml_lstm.yaml')))
    assert masked['maml_lengths'] is True and 'maml_lengths' not in base and 'mask_padding' not in masked
    assert {k: v for k, v in masked.items() if k not in ('name', 'maml_lengths')} == {k: v for k, v in base.items() if k != 'name'}
