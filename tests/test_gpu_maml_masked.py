"""-m gpu: the MAML-style step with per-song lengths (include/fsmg.h "cfg-E with per-song lengths").

The shapes are maml_ref.MAML_SHAPES, the lengths maml_masked_ref.lengths_of: every set of two rows or more holds a 1 and a max_len,
and n_valid_sup != n_valid_qry, so swapped length arrays cannot pass.  (Shape 0 has ONE row per set, which cannot hold both: its
rows get a length strictly between.)

Laws, bitwise, against the verified unmasked (tests/test_gpu_maml_componentwise.py) and one-pass masked (tests/test_masked.py) paths:
  L1  full lengths give the unmasked MAML call's bits;
  L2  the tokens behind a song's end never matter;
  L3  with inner_steps = 0 the calls are the one-pass masked calls on the query rows;
  L4  the indexed forms are the token forms on the gathered rows and lengths; refusals leave everything as it was;
  L5  eval, score and generate adapt to the train form's theta' bits, which are not the unmasked adaptation's.
Against fp64 (tests/maml_masked_ref.py), with the bounds of tests/test_gpu_maml_componentwise.py and no new numbers: theta' of every
inner step through maml_ref.sgd_check from the device's own masked gradient, the query loss to NLL_RTOL, theta' and the outer
gradients to REL_MAX; the masked rows of dlogits are exact zeros.  Then the forced time-out, alternation under graph replay, and
the plugin on the golden lyrics.
"""
import os

import numpy as np
import pytest
import yaml

import maml_masked_ref as MM
import maml_ref as MR
import masked_ref as KR
from gpu_utils import new_model, rel_max
from test_gpu_maml_componentwise import NLL_RTOL, REL_MAX, adapted, assert_same_bits, handle
from test_maml_paths import assert_same_state, songs, state

pytestmark = pytest.mark.gpu

LR = MR.INNER_LR
NONE = np.zeros(1, np.int32)[:0]            # the lengths of no rows (a pass over one set only)
SMALLEST, H512 = 0, 3                       # the smallest shape; hidden 512 with two inner steps (the fp32 XCD-local kernels)
PATHS = {'default': {}, 'serial': {'FSMG_XCD_OVERLAP': '0'}, 'ce_pass': {'FSMG_FUSED_SOFTMAX': '0'}}      # tests/test_masked.py's


def case(idx):
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape)
    T = cfg['max_len']
    sup, qry = MR.episode(cfg, shape)
    sl, ql = MM.lengths_of(shape, T)
    for ln in (sl, ql):
        assert ln.dtype == np.int32 and ((ln.min() == 1 and ln.max() == T) if ln.size > 1 else 1 < ln.min() < T)
    assert int(sl.sum()) != int(ql.sum())
    return shape, cfg, sup.astype(np.int32), qry.astype(np.int32), sl, ql


def scrambled(cfg, sup, qry, sl, ql):
    rng = np.random.RandomState(91)
    sup2, qry2 = KR.scramble_padding(sup, sl, cfg['input_size'], rng), KR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) and not np.array_equal(qry, qry2)
    return sup2, qry2


def snapshot(model, run):
    """a _forward_backward call through `run`, then the update: loss, every outer gradient, tail, theta', parameters, Adam slots"""
    before = model.get_params()
    run(model)
    out = {'grad:' + k: model.get_grad(k).copy() for k in model.param_shapes}
    out['tail'] = model.debug_read('tail', 16)[:2].copy()           # squared norm of the embedding slices, loss
    for k, v in adapted(model).items():
        out['adapted:' + k] = v.copy()
    assert_same_bits(model.get_params(), before, 'theta after the call')
    out['loss'] = np.float32(model.apply_update(1.0))
    for k in model.param_shapes:
        out['param:' + k] = model.get_param(k).copy()
        m, v = model.get_opt_state(k)
        out['m:' + k], out['v:' + k] = m.copy(), v.copy()
    out['step'] = np.int64(model.step)
    return out


def same(a, b, what=''):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), (what, k)


def rows_pass(model, rows, lens):
    """one masked pass over one set's rows: what the masked adaptation runs per inner step, and for the query rows at theta'"""
    N, R = rows.shape[:2]
    model.forward_backward_masked(rows, rows, lens, NONE, shape=(N, R, 0))


# ----------------------------------------------------------------------------- L1
@pytest.mark.parametrize('idx,path', [(SMALLEST, p) for p in PATHS] + [(H512, p) for p in PATHS], ids=str)
def test_full_lengths_are_the_unmasked_call_bit_for_bit(idx, path, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    shape, cfg, sup, qry, sl, ql = case(idx)
    n, T = shape[4], cfg['max_len']
    fs, fq = np.full_like(sl, T), np.full_like(ql, T)
    theta = MR.initial_theta(cfg)
    a = snapshot(handle(cfg, theta, shape), lambda m: m.maml_forward_backward(sup, qry, n, LR))
    b = snapshot(handle(cfg, theta, shape), lambda m: m.maml_forward_backward_masked(sup, qry, fs, fq, n, LR))
    same(a, b, 'maml_forward_backward_masked')
    assert max(rel_max(a['adapted:' + k], theta[k]) for k in theta if not k.startswith('bias_')) > 1e-3      # theta', not theta
    u, m = handle(cfg, theta, shape), handle(cfg, theta, shape)
    for s in range(2):
        lu, lm = u.maml_step(sup, qry, n, LR), m.maml_step_masked(sup, qry, fs, fq, n, LR)
        assert np.float32(lu) == np.float32(lm) and (s > 0 or np.float32(lm) == a['loss'])
        assert_same_state(state(u), state(m), 'maml_step_masked %d' % s)
        assert_same_bits(adapted(m), adapted(u), 'theta-prime of step %d' % s)
        if s == 0:                               # ... which is the split form's update
            same({k: v for k, v in a.items() if k[:2] in ('pa', 'm:', 'v:')}, snapshot_state(m, lambda h: None), 'first step')
    assert np.float32(u.maml_eval(sup, qry, n, LR)) == np.float32(m.maml_eval_masked(sup, qry, fs, fq, n, LR))
    assert_same_state(state(u), state(m), 'after maml_eval_masked')
    assert u.stats()['timeouts'] == 0 and m.stats()['timeouts'] == 0 and m.step == 2


def snapshot_state(model, run):
    run(model)
    out = {}
    for k in model.param_shapes:
        out['param:' + k] = model.get_param(k).copy()
        m, v = model.get_opt_state(k)
        out['m:' + k], out['v:' + k] = m.copy(), v.copy()
    return out


# ----------------------------------------------------------------------------- L2
@pytest.mark.parametrize('idx', [1, H512])
def test_padding_never_matters(idx):
    shape, cfg, sup, qry, sl, ql = case(idx)
    n, T = shape[4], cfg['max_len']
    over, N, K, Q = shape[:4]
    sup2, qry2 = scrambled(cfg, sup, qry, sl, ql)
    theta = MR.initial_theta(cfg)
    flat_len, q_len = sl.reshape(-1), ql.reshape(-1)

    def everything(s, q):
        m = handle(cfg, theta, shape)
        out = snapshot(m, lambda h: h.maml_forward_backward_masked(s, q, sl, ql, n, LR))
        out['step_loss'] = np.float32(m.maml_step_masked(s, q, sl, ql, n, LR))
        out.update({'2:' + k: v for k, v in snapshot_state(m, lambda h: None).items()})
        out['nll'] = np.float32(m.maml_eval_masked(s, q, sl, ql, n, LR))
        sc = m.maml_score(s.reshape(N * K, T), q.reshape(N * Q, T), n, LR, rank=True, entropy=True, argmax=True,
                          support_len=flat_len, lengths=q_len)
        out.update({'score:' + k: v for k, v in sc.items()})
        toks, lp = m.maml_generate(s.reshape(N * K, T), 4, n, LR, n_seq=3, seed=5, logprobs=True, support_len=flat_len)
        out['gen:tokens'], out['gen:logprob'] = toks, lp
        btoks, bscores = m.maml_beam_search(s.reshape(N * K, T), 3, n, LR, 2, support_len=flat_len)
        out['beam:tokens'], out['beam:scores'] = btoks, bscores
        assert m.stats()['timeouts'] == 0
        return out
    a, b = everything(sup, qry), everything(sup2, qry2)
    same(a, b)
    # ... and the mask is not a no-op: the unmasked call of the same episode differs
    c = snapshot(handle(cfg, theta, shape), lambda h: h.maml_forward_backward(sup, qry, n, LR))
    assert c['loss'] != a['loss'] and not np.array_equal(c['grad:softmax_w'], a['grad:softmax_w'])
    assert not np.array_equal(c['adapted:softmax_w'], a['adapted:softmax_w'])


# ----------------------------------------------------------------------------- L3
@pytest.mark.parametrize('idx', [1, H512])
def test_without_inner_steps_the_calls_are_the_one_pass_masked_calls(idx):
    shape, cfg, sup, qry, sl, ql = case(idx)
    over, N, K, Q = shape[:4]
    theta = MR.initial_theta(cfg)

    def grads(m):
        out = {k: m.get_grad(k).copy() for k in m.param_shapes}
        out['tail'] = m.debug_read('tail', 16)[:2].copy()
        return out
    a, b = handle(cfg, theta, shape), handle(cfg, theta, shape, keep=False)
    a.maml_forward_backward_masked(sup, qry, sl, ql, 0, LR)
    b.forward_backward_masked(qry, qry, NONE, ql, shape=(N, 0, Q))         # K = 0: the query rows and their lengths alone
    same(grads(a), grads(b), 'K = 0')
    assert_same_bits(adapted(a), theta, 'no inner step: theta-prime is theta')
    assert np.float32(a.apply_update(1.0)) == np.float32(b.apply_update(1.0))
    assert_same_state(state(a), state(b))
    assert np.float32(a.maml_eval_masked(sup, qry, sl, ql, 0, LR)) == np.float32(b.eval_step_masked(qry, ql))


# ----------------------------------------------------------------------------- L4
@pytest.mark.parametrize('idx', [1, H512])
def test_indexed_forms_equal_the_token_forms_and_refusals_touch_nothing(idx):
    from fsmg.binding import FsmgError
    shape, cfg, sup, qry, sl, ql = case(idx)
    over, N, K, Q, n, seed = shape
    T, B = cfg['max_len'], N * (K + Q)
    theta = MR.initial_theta(cfg)
    table = songs(cfg, 40, seed=5)
    rng = np.random.RandomState(7)
    table_len = KR.lengths_for(rng, (40,), T)
    a, b = new_model(cfg, theta, max_sequences=B), new_model(cfg, theta, max_sequences=B)
    b.upload_table(0, table, table_len)
    b.upload_table(1, table)                                               # a table without lengths
    for s in range(2):
        si, qi = rng.randint(0, 40, size=(N, K)), rng.randint(0, 40, size=(N, Q))
        si[0, 0] = 39                                                      # the last row of the table
        qi[N - 1, Q - 1] = si[N - 1, K - 1]                                # a song twice, in both sets
        want = a.maml_step_masked(table[si], table[qi], table_len[si], table_len[qi], n, LR)
        got = b.maml_step_indexed_masked(0, si, qi, n, LR, want_loss=(s != 1))
        assert got == (want if s != 1 else None)
        assert_same_state(state(a), state(b), 'step %d' % s)
    np.testing.assert_array_equal(b.read_losses(2), a.read_losses(2))
    si, qi = rng.randint(0, 40, size=(N + 2, K)), rng.randint(0, 40, size=(N + 2, Q))      # more rows than the handle has seen
    before = state(b)
    a.maml_forward_backward_masked(table[si], table[qi], table_len[si], table_len[qi], n, LR)
    b.maml_forward_backward_indexed_masked(0, si, qi, n, LR)
    for k in a.param_shapes:
        ga, gb = a.get_grad(k), b.get_grad(k)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)) and np.abs(ga).max() > 0, k
    assert_same_state(state(b), before, 'theta untouched')
    assert_same_state(state(a), before)
    # the refusals: a table without lengths, no table, a host length outside [1, max_len] in either set, a missing pointer
    si, qi = si[:N], qi[:N]
    bad_s, bad_q = sl.copy(), ql.copy()
    bad_s[N - 1, K - 1], bad_q[0, 0] = T + 1, 0
    b.debug_set('keep_adapted', 1)
    b.maml_eval_masked(sup, qry, sl, ql, n, LR)
    kept = adapted(b)
    for what, code, call in [
            ('table without lengths', 'STATE', lambda: b.maml_step_indexed_masked(1, si, qi, n, LR)),
            ('table without lengths, split', 'STATE', lambda: b.maml_forward_backward_indexed_masked(1, si, qi, n, LR)),
            ('no table', 'STATE', lambda: b.maml_step_indexed_masked(2, si, qi, n, LR)),
            ('support length T + 1', 'INVALID', lambda: b.maml_step_masked(sup, qry, bad_s, ql, n, LR)),
            ('query length 0', 'INVALID', lambda: b.maml_forward_backward_masked(sup, qry, sl, bad_q, n, LR)),
            ('query length 0, eval', 'INVALID', lambda: b.maml_eval_masked(sup, qry, sl, bad_q, n, LR)),
            ('support length T + 1, score', 'INVALID',
             lambda: b.maml_score(sup.reshape(N * K, T), qry.reshape(N * Q, T), n, LR, support_len=bad_s.reshape(-1))),
            ('support length T + 1, generate', 'INVALID',
             lambda: b.maml_generate(sup.reshape(N * K, T), 3, n, LR, support_len=bad_s.reshape(-1))),
            ('support length T + 1, beam search', 'INVALID',
             lambda: b.maml_beam_search(sup.reshape(N * K, T), 3, n, LR, 2, support_len=bad_s.reshape(-1)))]:
        with pytest.raises(FsmgError, match=code):
            call()
        assert_same_state(state(b), before, what)
        assert_same_bits(adapted(b), kept, what + ': the kept theta-prime')          # not even the adaptation began
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0
    assert a.maml_step_masked(sup, qry, sl, ql, n, LR) == b.maml_step_masked(sup, qry, sl, ql, n, LR)       # the handle goes on
    assert_same_state(state(a), state(b), 'the next good step')


# ----------------------------------------------------------------------------- device-resident tokens and lengths
def test_device_resident_tokens_and_lengths():
    """tokens_on_device / support_on_device cover the lengths too; a device length outside [1, max_len] meets the range check of the
    kernel that builds the weights: TOKEN_RANGE from every entry point, everything as it was"""
    import torch
    from fsmg.binding import FsmgError
    shape, cfg, sup, qry, sl, ql = case(1)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    theta = MR.initial_theta(cfg)
    a, b = handle(cfg, theta, shape), handle(cfg, theta, shape)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (sup, qry, sl, ql)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in dev]
    for s in range(2):
        assert np.float32(a.maml_step_masked(sup, qry, sl, ql, n, LR)) == np.float32(b.maml_step_masked(*ptr, n, LR, shape=(N, K, Q)))
        assert_same_state(state(a), state(b), 'step %d' % s)
    assert np.float32(a.maml_eval_masked(sup, qry, sl, ql, n, LR)) == np.float32(b.maml_eval_masked(*ptr, n, LR, shape=(N, K, Q)))
    a.maml_forward_backward_masked(sup, qry, sl, ql, n, LR)
    b.maml_forward_backward_masked(*ptr, n, LR, shape=(N, K, Q))
    for k in a.param_shapes:
        assert np.array_equal(a.get_grad(k).view(np.uint32), b.get_grad(k).view(np.uint32)), k
    flat, flat_len, songs_q = sup.reshape(N * K, T), sl.reshape(-1), qry.reshape(N * Q, T)
    ga = a.maml_generate(flat, 4, n, LR, n_seq=2, seed=3, support_len=flat_len)
    gb = b.maml_generate(ptr[0], 4, n, LR, n_seq=2, seed=3, n_support_rows=N * K, support_len=ptr[2])
    np.testing.assert_array_equal(ga, gb)
    same(a.maml_score(flat, songs_q, n, LR, support_len=flat_len), b.maml_score(ptr[0], songs_q, n, LR, n_support_rows=N * K, support_len=ptr[2]))
    assert_same_bits(adapted(b), adapted(a), 'theta-prime from device-resident support rows and lengths')
    before = state(b)
    for which, wrong in ((2, 0), (2, T + 1), (3, T + 1)):
        bad = (sl if which == 2 else ql).copy()
        bad[N - 1, 0] = wrong
        d_bad = torch.from_numpy(bad).cuda()
        torch.cuda.synchronize()
        p = list(ptr)
        p[which] = d_bad.data_ptr()
        calls = [lambda: b.maml_step_masked(*p, n, LR, shape=(N, K, Q)), lambda: b.maml_eval_masked(*p, n, LR, shape=(N, K, Q))]
        if which == 2:
            calls += [lambda: b.maml_generate(ptr[0], 4, n, LR, n_support_rows=N * K, support_len=p[2]),
                      lambda: b.maml_beam_search(ptr[0], 3, n, LR, 2, n_support_rows=N * K, support_len=p[2]),
                      lambda: b.maml_score(ptr[0], songs_q, n, LR, n_support_rows=N * K, support_len=p[2])]
        for i, call in enumerate(calls):
            with pytest.raises(FsmgError, match='TOKEN_RANGE'):
                call()
            assert_same_state(state(b), before, 'device length %d, call %d' % (wrong, i))
    # the handle goes on as if nothing had happened
    assert np.float32(a.maml_step_masked(sup, qry, sl, ql, n, LR)) == np.float32(b.maml_step_masked(*ptr, n, LR, shape=(N, K, Q)))
    assert_same_state(state(a), state(b), 'the next good step')
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- L5
@pytest.mark.parametrize('idx', [1, H512])
def test_eval_score_and_generate_adapt_to_the_same_bits(idx):
    shape, cfg, sup, qry, sl, ql = case(idx)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    theta = MR.initial_theta(cfg)
    a = handle(cfg, theta, shape)
    a.maml_forward_backward_masked(sup, qry, sl, ql, n, LR)
    want = adapted(a)
    u = handle(cfg, theta, shape)
    u.maml_forward_backward(sup, qry, n, LR)
    unmasked = adapted(u)
    assert any(not np.array_equal(want[k], unmasked[k]) for k in want)          # the lengths arrive
    assert max(rel_max(want[k], unmasked[k]) for k in want if not k.startswith('bias_')) > 1e-4
    flat, flat_len = sup.reshape(N * K, T), sl.reshape(-1)
    calls = [('maml_eval_masked', lambda m: m.maml_eval_masked(sup, qry, sl, ql, n, LR)),
             ('maml_score', lambda m: m.maml_score(flat, qry.reshape(N * Q, T), n, LR, support_len=flat_len)),
             ('maml_generate', lambda m: m.maml_generate(flat, 4, n, LR, n_seq=2, seed=1, support_len=flat_len)),
             ('maml_beam_search', lambda m: m.maml_beam_search(flat, 3, n, LR, 2, support_len=flat_len))]
    for name, call in calls:
        m = handle(cfg, theta, shape)
        call(m)
        assert_same_bits(adapted(m), want, name)
        assert_same_bits(m.get_params(), theta, name + ': theta afterwards')
        assert m.stats()['timeouts'] == 0
        call(a)                                                                  # ... and on the handle that has run the train form before
        assert_same_bits(adapted(a), want, name + ' after maml_forward_backward_masked')
        assert_same_bits(a.get_params(), theta, name + ': theta afterwards')
    # what runs at theta' is the unmasked twin's work: at full lengths the decoders return the twin's bits
    full = np.full_like(flat_len, T)
    np.testing.assert_array_equal(a.maml_generate(flat, 4, n, LR, n_seq=2, seed=1, support_len=full), u.maml_generate(flat, 4, n, LR, n_seq=2, seed=1))
    sa, su = a.maml_score(flat, qry.reshape(N * Q, T), n, LR, support_len=full), u.maml_score(flat, qry.reshape(N * Q, T), n, LR)
    same(sa, su, 'maml_score at full lengths')
    assert a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- against fp64
_REF = {}


def reference(idx, mode):
    """maml_masked_ref.query_grads in fp64: computed once per (shape, mode), never written to"""
    if (idx, mode) not in _REF:
        shape, cfg, sup, qry, sl, ql = case(idx)
        _REF[(idx, mode)] = MM.query_grads(MR.f64(MR.initial_theta(cfg)), sup, qry, sl, ql, cfg, shape[4], LR, mode)
    return _REF[(idx, mode)]


FP64_CASES = [(i, 'tf1_slices') for i in range(len(MR.MAML_SHAPES))] + [(1, 'dense'), (H512, 'dense')]


@pytest.mark.parametrize('idx,mode', FP64_CASES, ids=str)
def test_every_inner_step_and_the_query_pass_against_fp64(idx, mode):
    shape, cfg, sup, qry, sl, ql = case(idx)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    theta = MR.initial_theta(cfg)
    a, b = handle(cfg, theta, shape, mode), handle(cfg, theta, shape, mode, keep=False)
    a.debug_set('inplace_dlogits', 0)
    b.debug_set('inplace_dlogits', 0)
    V1p = a.debug_dims()['V1p']

    def masked_rows_of_dlogits_are_zero(m, ln, rows):
        assert m.debug_read('fused_softmax', 2)[1] == 0                          # dlogits was materialised
        d = m.debug_read('dlogits', rows * T * V1p).reshape(T, rows, V1p)       # device row order t * B + b
        pad = np.arange(T)[:, None] >= ln.reshape(-1)[None, :]
        assert pad.any() and np.all(d[pad] == 0) and np.all(np.abs(d[~pad]).max(axis=-1) > 0)
    label = 'masked|%s|%s' % (MR.shape_id(shape), mode)
    prev, failures = a.get_params(), []
    for i in range(1, n + 1):
        a.maml_forward_backward_masked(sup, qry, sl, ql, i, LR)                  # from the same theta each time: it restores
        got_gnorm = float(a.debug_read('gnorm', 1)[0])
        theta_i = adapted(a)
        assert_same_bits(a.get_params(), theta, 'theta after the call')
        b.set_params(prev)
        rows_pass(b, sup, sl)                                                    # the inner pass, by fsmg_forward_backward_masked
        masked_rows_of_dlogits_are_zero(b, sl, N * K)
        grads = {k: b.get_grad(k) for k in b.param_shapes}
        gnorm, step, bad = MR.sgd_check('%s|%d' % (label, i), prev, grads, b.debug_read('tail', 16), mode, cfg['max_grad_norm'], LR,
                                        theta_i, got_gnorm)
        failures += ['step %d: %s' % (i, f) for f in bad]
        assert gnorm > cfg['max_grad_norm'] and got_gnorm > cfg['max_grad_norm']            # the clip is active (fp64: 0.68 .. 0.73 against 0.3)
        prev = theta_i
    assert not failures, '%s: %s' % (label, '; '.join(failures))
    masked_rows_of_dlogits_are_zero(a, ql, N * Q)                                # the query pass of the MAML call itself
    # the query pass is the one-pass masked call at theta'
    b.set_params(prev)
    rows_pass(b, qry, ql)
    for k in a.param_shapes:
        assert np.array_equal(a.get_grad(k).view(np.uint32), b.get_grad(k).view(np.uint32)), k
    ref = reference(idx, mode)
    loss = float(a.debug_read('tail', 16)[1])
    print('FP64|%s|loss %.9g want %.9g rel %.2e' % (label, loss, ref['loss'], abs(loss - ref['loss']) / abs(ref['loss'])))
    for k in sorted(ref['theta']):
        print('FP64|%s|%s|theta %.2e|gradient %.2e' % (label, k, rel_max(prev[k], ref['theta'][k]), rel_max(a.get_grad(k), ref['grads'][k])))
    assert abs(loss - ref['loss']) <= NLL_RTOL * abs(ref['loss']), (loss, ref['loss'])
    for k in ref['theta']:
        assert rel_max(prev[k], ref['theta'][k]) < REL_MAX, ('theta', k)
        assert rel_max(a.get_grad(k), ref['grads'][k]) < REL_MAX, ('gradient', k)
    nll = a.maml_eval_masked(sup, qry, sl, ql, n, LR)
    assert abs(nll - ref['loss']) <= NLL_RTOL * abs(ref['loss']), (nll, ref['loss'])
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- the forced time-out
def test_timed_out_chain_inside_the_masked_eval_and_step():
    shape, cfg, sup, qry, sl, ql = case(H512)
    over, N, K, Q, n, seed = shape
    theta = MR.initial_theta(cfg)
    B = N * (K + Q)
    a, b = new_model(cfg, theta, max_sequences=B), new_model(cfg, theta, max_sequences=B)
    assert a.maml_step_masked(sup, qry, sl, ql, n, LR) == b.maml_step_masked(sup, qry, sl, ql, n, LR)
    st = a.stats()
    assert st['xcd_launches'] + st['persistent_launches'] > 0 and st['timeouts'] == 0 and st['persistent_path']
    want = b.maml_eval_masked(sup, qry, sl, ql, n, LR)                          # the NLL without a time-out
    unadapted = b.eval_step_masked(qry, ql)
    before = state(a)
    a.debug_set('chain_spin_limit', 0)          # tests/test_maml_paths.py's knob: the persistent kernels give up at their first wait
    got = a.maml_eval_masked(sup, qry, sl, ql, n, LR)                           # times out in the adaptation, repeated once with the lengths
    st = a.stats()
    assert st['timeouts'] == 1 and not st['persistent_path']
    assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
    assert abs(got - unadapted) > 10 * NLL_RTOL * abs(want), (got, unadapted)   # not the repeated chunk at the unadapted theta
    assert_same_state(state(a), before, 'maml_eval_masked under the time-out')
    b.debug_set('persistent', 0)                # what the repeat runs on
    assert got == b.maml_eval_masked(sup, qry, sl, ql, n, LR)
    a.debug_set('persistent', 1)                # back on the persistent kernels, which give up again: the is_retry route of the step
    assert a.maml_step_masked(sup, qry, sl, ql, n, LR) == b.maml_step_masked(sup, qry, sl, ql, n, LR)
    assert_same_state(state(a), state(b), 'the repeated masked step')
    st = a.stats()
    assert st['timeouts'] == 2 and st['steps_skipped_timeout'] == 1 and a.step == before[2] + 1


# ----------------------------------------------------------------------------- alternation under graph replay
def test_masked_and_unmasked_calls_alternate_on_one_handle_under_graph_replay(monkeypatch):
    monkeypatch.setenv('FSMG_EAGER', '0')
    shape, cfg, sup, qry, sl, ql = case(1)
    over, N, K, Q, n, seed = shape
    theta = MR.initial_theta(cfg)

    def make():
        m = new_model(cfg, theta, max_sequences=N * (K + Q), use_graph=True)
        m.debug_set('keep_adapted', 1)
        return m

    def run(m, kind):
        if kind == 'maml':
            m.maml_forward_backward(sup, qry, n, LR)
        elif kind == 'maml_masked':
            m.maml_forward_backward_masked(sup, qry, sl, ql, n, LR)
        elif kind == 'rows_masked':             # the one-pass masked call with the masked adaptation's own row counts: its graph key
            rows_pass(m, sup, sl)
        else:                                   # the pass the unmasked adaptation makes
            m.forward_backward(sup, sup, shape=(N, K, 0))
        out = {k: m.get_grad(k).copy() for k in m.param_shapes}
        out['tail'] = m.debug_read('tail', 16)[:2].copy()
        if kind.startswith('maml'):
            out.update({'adapted:' + k: v for k, v in adapted(m).items()})
            out['nll'] = np.float32(m.maml_eval(sup, qry, n, LR) if kind == 'maml' else m.maml_eval_masked(sup, qry, sl, ql, n, LR))
        return out
    kinds = ['maml', 'maml_masked', 'rows_masked', 'rows']
    alone = {k: run(make(), k) for k in kinds}
    one = make()
    for k in kinds + kinds[::-1] + ['maml_masked', 'maml_masked']:          # captures, then replays in another order
        same(run(one, k), alone[k], k)
    assert not np.array_equal(alone['maml']['tail'], alone['maml_masked']['tail'])
    assert one.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- the plugin
def test_plugin_with_maml_lengths_on_the_golden_lyrics(tmp_path, golden_dir, capsys):
    """config/maml_masked_lstm.yaml's key through train.train on both calling conventions: the window means it prints are the fp64
    restatement's on the same sampler stream, and not the unmasked oracle's"""
    import train.train as TT
    from conftest import ROOT
    from data.episode import load_sampler_from_config
    from models.maml_lstm import MAMLLSTM
    from oracle import lstm_oracle as O
    from test_masked_cpu import K, Q, T, _dataset, _raw_tree
    from test_train_entry import LOOP
    shipped = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'maml_masked_lstm.yaml')))
    assert shipped['maml_lengths'] is True and shipped['model_class_name'] == 'MAMLLSTM'
    # the golden tree ships token sidecars without lengths (every song then counts as max_len long): tokenise the raw songs once
    # with the whitespace tokenizer, as tests/test_masked_cpu.py does -- both sidecars of every song, vocabulary, splits
    root = _raw_tree(tmp_path, golden_dir)
    _dataset(root)[0].metadata.close()
    cfg = dict(LOOP, name='maml_masked_lstm', model_module_name=shipped['model_module_name'], model_class_name=shipped['model_class_name'],
               maml_lengths=shipped['maml_lengths'], n_train=4, print_every_n=2, val_every_n=4.0, n_val=2, n_test=2, n_samples=1,
               n_decay=10000, lr=5e-3, max_grad_norm=5, embedding_size=32, hidden_size=40, n_layers=1, inner_steps=1, inner_lr=0.3)
    docs = {'data': dict(dataset='lyrics', dataset_path=root, splits=['train', 'val', 'test'], max_len=T),
            'task': dict(query_size=Q, support_size=K, seed=1234), 'model': cfg}
    p = {}
    for name, doc in docs.items():
        p[name] = str(tmp_path / (name + '.yaml'))
        with open(p[name], 'w') as f:
            yaml.safe_dump(doc, f)
    full = {}
    for k in ('data', 'task', 'model'):
        full.update(yaml.safe_load(open(p[k])))
    full['split'] = 'train'
    sampler = load_sampler_from_config(dict(full))
    full['input_size'] = sampler.get_num_unique_words()
    probe = MAMLLSTM(dict(full))
    probe.recover_or_init('')
    params = {k: v.astype(np.float64) for k, v in probe.engine.get_params().items()}
    plain_params = {k: v.copy() for k, v in params.items()}
    opt, plain_opt = O.new_opt_state(params), O.new_opt_state(plain_params)
    want, plain, short = [], [], 0
    for _ in range(4):
        ep = sampler.get_episode()
        short += int((ep.support_len < full['max_len']).sum() + (ep.query_len < full['max_len']).sum())
        want.append(MM.maml_step(params, opt, ep.support, ep.query, ep.support_len, ep.query_len, full, 1, 0.3))
        plain.append(O.maml_step(plain_params, plain_opt, ep.support, ep.query, full, 1, 0.3))
    assert short > 0
    # the plugin's own calls on one episode: the binding's masked calls, and a missing length is a ValueError
    from data.episode import Episode
    raw = new_model(full, probe.engine.get_params(), max_sequences=ep.support.shape[0] * (ep.support.shape[1] + ep.query.shape[1]), use_graph=True)
    assert np.float32(probe.eval(ep)) == np.float32(raw.maml_eval_masked(ep.support, ep.query, ep.support_len, ep.query_len, 1, 0.3))
    assert np.float32(probe.train(ep)) == np.float32(raw.maml_step_masked(ep.support, ep.query, ep.support_len, ep.query_len, 1, 0.3))
    with pytest.raises(ValueError, match='length'):
        probe.train(Episode(ep.support, ep.query))
    with pytest.raises(ValueError, match='length'):
        probe.eval(Episode(ep.support, ep.query))
    out = {}
    for sync in ('0', '1'):
        os.environ['FSMG_TRAIN_SYNC'] = sync
        try:
            TT.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', str(tmp_path / ('ck' + sync))])
        finally:
            del os.environ['FSMG_TRAIN_SYNC']
        out[sync] = [l for l in capsys.readouterr().out.splitlines() if l.startswith('Iter: ') or 'Avg NLL' in l]
    assert out['0'] == out['1']                                    # the indexed route == the token route
    got = [float(l.split('loss: ')[1]) for l in out['0'] if ', loss: ' in l]
    assert len(got) == 2
    for g, w in zip(got, (np.mean(want[:2]), np.mean(want[2:]))):
        assert abs(g - w) <= 2e-3 * abs(w), (got, want)           # printed with 4 significant digits (tests/test_train_entry.py)
    assert abs(np.mean(plain[:2]) - np.mean(want[:2])) > 5e-3 * abs(np.mean(want[:2]))      # the check has teeth
