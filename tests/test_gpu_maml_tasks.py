"""-m gpu: per-artist MAML (include/fsmg.h "per-artist MAML"; references, bounds and shapes in tests/maml_tasks_ref.py).

  T1  N == 1: every tasks call has the bits of its fsmg_maml_* twin -- gradients, the 16 tail words, theta', parameters, Adam slots,
      global_step, loss and NLL -- in both clip modes, with lengths against the _masked twins.
  T2  composition: the tasks gradient is the float32 fold of N separate fsmg_maml_forward_backward(N = 1) results -- bitwise where N
      is a power of two (w * g exact), within one fp32 rounding per folded artist of their fp64 fold otherwise; tail[0], tail[1] and
      task_loss likewise.
  T3  against fp64 at every shape, both clip modes: the loss to NLL_RTOL, every tensor to 5e-4 * sum_n w max|g_n_ref|; the joint
      fsmg_maml_forward_backward of the same episode is more than 10 of those bounds away (B to F).
  T4  fsmg_maml_tasks_step against the oracle's update of the reference gradient; fsmg_maml_tasks_eval is the fp64 mean, rounded once,
      of N fsmg_maml_eval(N = 1) results.
  T5  lengths: all max_len gives the unmasked bits, the tokens behind a song's end never matter, ragged lengths against fp64.
  T6  table_id >= 0, with and without the table's lengths: the token form's bits.
  T7  Meta-SGD: GA is the fold of the separate calls' rate gradients; disabled again, the earlier bits.
  T8  state and errors: theta back, slots and step untouched, what is pending, every argument error with nothing touched, a token out
      of range in artist 1, a timed-out chain.
  T9  the plugin key.
"""
import ctypes as C
import os

import numpy as np
import pytest

import maml_masked_ref as MM
import maml_ref as MR
import maml_tasks_ref as TR
import masked_ref as KR
import msgd_ref as SR
from gpu_utils import new_model, rel_max
from oracle import lstm_oracle as O
from test_gpu_maml_componentwise import adapted, assert_same_bits
from test_maml_paths import assert_same_state, songs, state

pytestmark = pytest.mark.gpu

LR = TR.LR
MODES = ['tf1_slices', 'dense']
_REF = {}


def setup(name, one_artist=False):
    shape = TR.SHAPES[name]
    if one_artist:
        shape = TR.cut_to_one_artist(shape)
    cfg = TR.config_of(shape)
    sup, qry = TR.episode(cfg, shape)
    return shape, cfg, sup, qry, MR.initial_theta(cfg)


def handle(name, shape, cfg, theta, mode='tf1_slices', keep=True):
    m = new_model(cfg, theta, max_sequences=TR.rows_of(name, shape), clip_norm_mode=mode)
    if keep:
        m.debug_set('keep_adapted', 1)
    return m


def reference(name, mode, masked=False):
    """the fp64 statement: computed once per (shape, mode, masked), never written to"""
    key = (name, mode, masked)
    if key not in _REF:
        shape, cfg, sup, qry, theta = setup(name)
        lengths = TR.lengths_of(shape, cfg['max_len']) if masked else None
        _REF[key] = TR.reference(MR.f64(theta), sup, qry, cfg, shape[4], LR, mode, lengths=lengths)
    return _REF[key]


def pending(m):
    """what a _forward_backward call leaves: every gradient, the 16 tail words, theta'"""
    out = {'grad:' + k: m.get_grad(k).copy() for k in m.param_shapes}
    out['tail'] = m.debug_read('tail', 16).copy()
    for k, v in adapted(m).items():
        out['adapted:' + k] = v.copy()
    return out


def same(a, b, what=''):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)), (what, k)


def result(m):
    t = m.debug_read('tail', 16)
    return dict(loss=float(t[1]), aux=float(t[0]), grads={k: m.get_grad(k) for k in m.param_shapes})


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- T1
@pytest.mark.parametrize('masked', [False, True], ids=['tokens', 'lengths'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['A', 'D'])
def test_one_artist_has_the_bits_of_the_existing_calls(name, mode, masked):
    shape, cfg, sup, qry, theta = setup(name, one_artist=True)
    over, N, K, Q, n, seed = shape
    assert N == 1
    sl, ql = TR.lengths_of(shape, cfg['max_len'])
    kw = dict(support_len=sl, query_len=ql) if masked else {}

    def twin_fb(m):
        return m.maml_forward_backward_masked(sup, qry, sl, ql, n, LR) if masked else m.maml_forward_backward(sup, qry, n, LR)

    def twin_step(m):
        return m.maml_step_masked(sup, qry, sl, ql, n, LR) if masked else m.maml_step(sup, qry, n, LR)

    def twin_eval(m):
        return m.maml_eval_masked(sup, qry, sl, ql, n, LR) if masked else m.maml_eval(sup, qry, n, LR)
    a, b = handle(name, shape, cfg, theta, mode), handle(name, shape, cfg, theta, mode)
    a.maml_tasks_forward_backward(sup, qry, n, LR, **kw)
    twin_fb(b)
    same(pending(a), pending(b), '_forward_backward')
    assert_same_bits(a.get_params(), theta, 'theta after the call')
    assert np.float32(a.debug_read('task_loss', 1)[0]) == np.float32(a.debug_read('tail', 16)[1])
    assert np.float32(a.apply_update(1.0)) == np.float32(b.apply_update(1.0))
    assert_same_state(state(a), state(b), 'the update behind _forward_backward')
    for s in range(2):
        (la, per), lb = a.maml_tasks_step(sup, qry, n, LR, task_loss=True, **kw), twin_step(b)
        assert np.float32(la) == np.float32(lb) and bits(per)[0] == bits(lb)
        assert_same_state(state(a), state(b), '_step %d' % s)
        assert_same_bits(adapted(a), adapted(b), 'theta-prime of step %d' % s)
    (na, per), nb = a.maml_tasks_eval(sup, qry, n, LR, task_nll=True, **kw), twin_eval(b)
    assert np.float32(na) == np.float32(nb) and bits(per)[0] == bits(nb)
    assert_same_state(state(a), state(b), 'after _eval')
    assert a.step == 3 and a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0
    np.testing.assert_array_equal(a.read_losses(3), b.read_losses(3))


# ----------------------------------------------------------------------------- T2
def separate_calls(b, sup, qry, n, rates=False):
    """N separate fsmg_maml_forward_backward(N = 1) calls on one handle state -> per artist (gradients, tail, theta', [GA])"""
    out = []
    for a in range(sup.shape[0]):
        b.maml_forward_backward(sup[a:a + 1], qry[a:a + 1], n, LR)
        one = dict(grads={k: b.get_grad(k).copy() for k in b.param_shapes}, tail=b.debug_read('tail', 16).copy(), theta=adapted(b))
        if rates:
            one['GA'] = {k: b.msgd_get_grad(k).copy() for k in b.param_shapes}
        out.append(one)
    return out


@pytest.mark.parametrize('name', ['B', 'D', 'C', 'E'])
def test_the_call_is_the_fold_of_separate_one_artist_calls(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    per = separate_calls(b, sup, qry, n)
    got, tail = {k: a.get_grad(k) for k in a.param_shapes}, a.debug_read('tail', 16)
    assert_same_bits(a.get_params(), theta, 'theta after the call')
    assert_same_bits(adapted(a), per[-1]['theta'], 'theta-prime of the last artist')
    task_loss = a.debug_read('task_loss', N)
    assert np.array_equal(bits(task_loss), bits([p['tail'][1] for p in per]))
    assert all(np.all(p['tail'][2:6] == 0) for p in per) and np.all(tail[2:6] == 0)
    if N & (N - 1) == 0:
        for k in got:
            xs = [p['grads'][k] for p in per]
            assert TR.exactness_holds(xs), k                     # no non-zero element below 2^-120: w * g is exact
            assert np.array_equal(bits(got[k]), bits(TR.fold32_pow2(xs, N))), k
        aux, loss = TR.fold_tail32([p['tail'] for p in per], N)
        assert bits(tail[0]) == bits(aux) and bits(tail[1]) == bits(loss)
        print('TASKS|fold|%s|N %d|bitwise' % (name, N))
    else:
        worst = 0.0
        for k in got:
            ref, bound = TR.rounding_bound([p['grads'][k] for p in per], N)
            frac = np.abs(got[k].astype(np.float64) - ref) / bound
            worst = max(worst, float(frac.max()))
            assert np.all(frac <= 1.0), (k, float(frac.max()))
        for i, power in ((0, 2), (1, 1)):
            w = float(np.float32(1.0 / N)) ** power if power == 1 else float(np.float32(np.float32(1.0 / N) * np.float32(1.0 / N)))
            ref = sum(w * float(p['tail'][i]) for p in per)
            assert abs(float(tail[i]) - ref) <= N * TR.U * sum(abs(w * float(p['tail'][i])) for p in per), i
        print('TASKS|fold|%s|N %d|worst %.3f of one rounding per folded artist' % (name, N, worst))
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T3
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(TR.SHAPES))
def test_against_the_fp64_statement(name, mode):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    ref = reference(name, mode)
    a = handle(name, shape, cfg, theta, mode)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    dist = TR.distance(ref, result(a))
    task_loss = a.debug_read('task_loss', N)
    worst = max(dist, key=dist.get)
    print('TASKS|fp64|%s|%s|worst %.4f of its bound (%s)' % (name, mode, dist[worst], worst))
    assert dist[worst] <= 1.0, dist
    assert np.all(np.abs(task_loss - ref['task_loss']) <= TR.NLL_RTOL * np.abs(ref['task_loss']))
    if N > 1:               # the feature is visible on the device: today's joint call is another computation
        a.maml_forward_backward(sup, qry, n, LR)
        joint = TR.distance(ref, result(a))
        print('TASKS|joint|%s|%s|%.1f bounds away (%s)' % (name, mode, max(joint.values()), max(joint, key=joint.get)))
        assert max(joint.values()) > 10.0, joint
    assert a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T4
@pytest.mark.parametrize('name', ['B', 'D'])
def test_step_matches_the_oracles_update_of_the_reference_gradient(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    ref = reference(name, 'tf1_slices')
    params = MR.f64(theta)
    opt = O.new_opt_state(params)
    O.apply_update(params, ref['grads'], dict(embedding_slices_sq=ref['aux']), opt, cfg, 'tf1_slices')
    a = handle(name, shape, cfg, theta)
    loss, per = a.maml_tasks_step(sup, qry, n, LR, task_loss=True)
    assert abs(loss - ref['loss']) <= TR.NLL_RTOL * abs(ref['loss'])
    assert np.all(np.abs(per - ref['task_loss']) <= TR.NLL_RTOL * np.abs(ref['task_loss']))
    assert a.step == 1 and np.float32(a.read_losses(1)[0]) == np.float32(loss)
    for k in params:
        m, v = a.get_opt_state(k)
        assert rel_max(a.get_param(k), params[k]) < TR.REL_MAX, ('parameter', k)
        assert rel_max(m, opt['m'][k]) < TR.REL_MAX and rel_max(v, opt['v'][k]) < TR.REL_MAX, ('Adam slots', k)
    # want_loss=False leaves the loss in the ring; the second step is the one a handle takes that asked for it
    b = handle(name, shape, cfg, theta)
    b.maml_tasks_step(sup, qry, n, LR)
    assert a.maml_tasks_step(qry, sup, n, LR, want_loss=False) is None
    lb = b.maml_tasks_step(qry, sup, n, LR)
    assert_same_state(state(a), state(b), 'want_loss=False')
    assert np.float32(a.read_losses(2)[1]) == np.float32(lb)


@pytest.mark.parametrize('masked', [False, True], ids=['tokens', 'lengths'])
@pytest.mark.parametrize('name', ['B', 'C', 'D', 'E'])
def test_eval_is_the_rounded_mean_of_one_artist_evals(name, masked):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    sl, ql = TR.lengths_of(shape, cfg['max_len'])
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    before = state(a)
    if masked:
        nll, per = a.maml_tasks_eval(sup, qry, n, LR, support_len=sl, query_len=ql, task_nll=True)
        want = [b.maml_eval_masked(sup[i:i + 1], qry[i:i + 1], sl[i:i + 1], ql[i:i + 1], n, LR) for i in range(N)]
    else:
        nll, per = a.maml_tasks_eval(sup, qry, n, LR, task_nll=True)
        want = [b.maml_eval(sup[i:i + 1], qry[i:i + 1], n, LR) for i in range(N)]
    assert np.array_equal(bits(per), bits(want))
    total = 0.0
    for w in want:
        total += float(np.float32(w))
    assert bits(nll) == bits(np.float32(total / N))
    assert_same_bits(adapted(a), adapted(b), 'theta-prime of the last artist')
    assert_same_state(state(a), before, 'after _eval')
    ref, ref_per = TR.eval_reference(MR.f64(theta), sup, qry, cfg, n, LR, lengths=(sl, ql) if masked else None)
    assert abs(nll - ref) <= TR.NLL_RTOL * abs(ref) and np.all(np.abs(per - ref_per) <= TR.NLL_RTOL * np.abs(ref_per))
    with pytest.raises(Exception, match='STATE'):
        a.apply_update(1.0)                                      # an evaluation leaves nothing pending
    assert a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T5
@pytest.mark.parametrize('name', ['B', 'D'])
def test_lengths_full_lengths_and_padding(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    sl, ql = TR.lengths_of(shape, T)
    fs, fq = np.full_like(sl, T), np.full_like(ql, T)
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    b.maml_tasks_forward_backward(sup, qry, n, LR, support_len=fs, query_len=fq)
    unmasked = pending(a)
    same(unmasked, pending(b), 'lengths all max_len')
    assert np.float32(a.maml_tasks_eval(sup, qry, n, LR)) == np.float32(b.maml_tasks_eval(sup, qry, n, LR, support_len=fs, query_len=fq))
    # the tokens behind a song's end do not matter
    rng = np.random.RandomState(91)
    sup2, qry2 = KR.scramble_padding(sup, sl, cfg['input_size'], rng), KR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) and not np.array_equal(qry, qry2)
    a.maml_tasks_forward_backward(sup, qry, n, LR, support_len=sl, query_len=ql)
    b.maml_tasks_forward_backward(sup2, qry2, n, LR, support_len=sl, query_len=ql)
    ragged = pending(a)
    same(ragged, pending(b), 'scrambled padding')
    assert not np.array_equal(ragged['grad:softmax_w'], unmasked['grad:softmax_w'])         # ... and the mask is not a no-op
    la, lb = a.maml_tasks_step(sup, qry, n, LR, support_len=sl, query_len=ql), b.maml_tasks_step(sup2, qry2, n, LR, support_len=sl, query_len=ql)
    assert np.float32(la) == np.float32(lb)
    assert_same_state(state(a), state(b), 'scrambled padding: the step')
    assert np.float32(a.maml_tasks_eval(sup, qry, n, LR, support_len=sl, query_len=ql)) == \
        np.float32(b.maml_tasks_eval(sup2, qry2, n, LR, support_len=sl, query_len=ql))
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


@pytest.mark.parametrize('name', list(TR.SHAPES))
def test_ragged_lengths_against_the_masked_fp64_statement(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    sl, ql = TR.lengths_of(shape, cfg['max_len'])
    ref = reference(name, 'tf1_slices', masked=True)
    a = handle(name, shape, cfg, theta)
    a.maml_tasks_forward_backward(sup, qry, n, LR, support_len=sl, query_len=ql)
    dist = TR.distance(ref, result(a))
    worst = max(dist, key=dist.get)
    print('TASKS|fp64-lengths|%s|worst %.4f of its bound (%s)' % (name, dist[worst], worst))
    assert dist[worst] <= 1.0, dist
    task_loss = a.debug_read('task_loss', N)
    assert np.all(np.abs(task_loss - ref['task_loss']) <= TR.NLL_RTOL * np.abs(ref['task_loss']))
    assert a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T6
@pytest.mark.parametrize('name', ['B', 'D'])
def test_table_forms_have_the_token_forms_bits(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    table = songs(cfg, 40, seed=5)
    rng = np.random.RandomState(7)
    table_len = KR.lengths_for(rng, (40,), T)
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    b.upload_table(0, table, table_len)
    b.upload_table(1, table)                                     # a table without lengths
    for lengths in (False, True):
        si, qi = rng.randint(0, 40, size=(N, K)), rng.randint(0, 40, size=(N, Q))
        si[0, 0] = 39                                            # the last row of the table
        qi[N - 1, Q - 1] = si[N - 1, K - 1]                      # a song twice, in both sets
        kw = dict(support_len=table_len[si], query_len=table_len[qi]) if lengths else {}
        a.maml_tasks_forward_backward(table[si], table[qi], n, LR, **kw)
        b.maml_tasks_forward_backward(si, qi, n, LR, table=0 if lengths else 1, table_lengths=lengths)
        same(pending(a), pending(b), '_forward_backward, lengths %s' % lengths)
        assert np.array_equal(bits(a.debug_read('task_loss', N)), bits(b.debug_read('task_loss', N)))
        la, lb = a.maml_tasks_step(table[si], table[qi], n, LR, **kw), b.maml_tasks_step(si, qi, n, LR, table=0, table_lengths=lengths)
        assert np.float32(la) == np.float32(lb)
        assert_same_state(state(a), state(b), '_step, lengths %s' % lengths)
        assert np.float32(a.maml_tasks_eval(table[si], table[qi], n, LR, **kw)) == \
            np.float32(b.maml_tasks_eval(si, qi, n, LR, table=0, table_lengths=lengths))
    before = state(b)
    for what, call in [('a table without lengths', lambda: b.maml_tasks_step(si, qi, n, LR, table=1, table_lengths=True)),
                       ('no table', lambda: b.maml_tasks_forward_backward(si, qi, n, LR, table=2)),
                       ('no table, eval', lambda: b.maml_tasks_eval(si, qi, n, LR, table=3))]:
        with pytest.raises(Exception, match='STATE'):
            call()
        assert_same_state(state(b), before, what)
    bad = si.copy()
    bad[1, 0] = 40                                               # one past the table, in artist 1
    with pytest.raises(Exception, match='TOKEN_RANGE'):
        b.maml_tasks_step(bad, qi, n, LR, table=0)
    assert_same_state(state(b), before, 'an index past the table')
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T7
@pytest.mark.parametrize('name', ['B', 'D'])
def test_meta_sgd_rate_gradient_is_the_fold(name):
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    rates = SR.draw_rates(cfg)
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    earlier = pending(a)
    for m in (a, b):
        m.msgd_enable(**SR.msgd_config())
        for k, v in rates.items():
            m.msgd_set_alpha(k, v)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    assert a.msgd_info()['pending']
    per = separate_calls(b, sup, qry, n, rates=True)
    for k in a.param_shapes:
        xs, gs = [p['GA'][k] for p in per], [p['grads'][k] for p in per]
        assert TR.exactness_holds(xs) and TR.exactness_holds(gs), k
        assert np.array_equal(bits(a.msgd_get_grad(k)), bits(TR.fold32_pow2(xs, N))), ('rate gradient', k)
        assert np.array_equal(bits(a.get_grad(k)), bits(TR.fold32_pow2(gs, N))), ('gradient', k)
        assert np.abs(a.msgd_get_grad(k)).max() > 0, k
    assert_same_bits(adapted(a), per[-1]['theta'], 'theta-prime of the last artist')
    assert not np.array_equal(adapted(a)['softmax_w'], earlier['adapted:softmax_w'])        # the rates are in the adaptation
    before = a.msgd_get_alphas()
    a.apply_update(1.0)                                          # the rates move with theta
    after = a.msgd_get_alphas()
    assert any(np.any(after[k] != before[k]) for k in after) and a.step == 1
    # disabled again: the bits of the handle that was never enabled (from the same theta)
    a.msgd_disable()
    a.set_params(theta)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    same(pending(a), earlier, 'disabled again')
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T8
def raw_call(m, fn, sup, qry, sl, ql, N, K, Q, extra=(), **fields):
    """the entry point `fn` with a config built field by field (what the binding never builds): -> status code"""
    from fsmg.binding import FsmgMamlTasksConfig
    cfg = FsmgMamlTasksConfig()
    cfg.struct_size, cfg.inner_steps, cfg.inner_lr, cfg.table_id = C.sizeof(FsmgMamlTasksConfig), 1, LR, -1
    for k, v in fields.items():
        if k == 'reserved':
            cfg.reserved[1] = v
        else:
            setattr(cfg, k, v)
    keep =[np.ascontiguousarray(x, np.int32) for x in (sup, qry, sl, ql) if x is not None]
    args = [C.c_void_p(k.ctypes.data) for k in keep]
    it = iter(args)
    p = [next(it) if x is not None else None for x in (sup, qry, sl, ql)]
    return getattr(m._lib, fn)(m._h, C.byref(cfg), p[0], p[1], p[2], p[3], N, K, Q, *extra)


def test_state_pending_and_argument_errors():
    name = 'B'
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    sl, ql = TR.lengths_of(shape, T)
    a = handle(name, shape, cfg, theta)
    a.maml_tasks_step(sup, qry, n, LR)                           # Adam slots that are not zero
    before = state(a)
    a.maml_tasks_forward_backward(sup, qry, n, LR)
    assert_same_state(state(a), before, 'after _forward_backward')
    kept = adapted(a)
    loss = np.float32(a.apply_update(1.0))                       # ... which left a gradient pending
    assert np.float32(a.read_losses(2)[1]) == loss and a.step == 2
    before = state(a)
    a.maml_tasks_eval(sup, qry, n, LR)
    assert_same_state(state(a), before, 'after _eval')
    with pytest.raises(Exception, match='STATE'):
        a.apply_update(1.0)
    kept = adapted(a)
    INVALID = -1
    nll, per = C.c_float(), (C.c_float * N)()
    outs = {'fsmg_maml_tasks_forward_backward': (), 'fsmg_maml_tasks_step': (C.byref(nll), per), 'fsmg_maml_tasks_eval': (C.byref(nll), per)}
    bad_s, bad_q = sl.copy(), ql.copy()
    bad_s[N - 1, K - 1], bad_q[0, 0] = T + 1, 0
    cases = [('struct_size', dict(struct_size=28), (sup, qry, None, None)), ('reserved', dict(reserved=1), (sup, qry, None, None)),
             ('inner_steps 65', dict(inner_steps=65), (sup, qry, None, None)), ('inner_steps -1', dict(inner_steps=-1), (sup, qry, None, None)),
             ('inner_lr < 0', dict(inner_lr=-0.5), (sup, qry, None, None)), ('inner_lr NaN', dict(inner_lr=float('nan')), (sup, qry, None, None)),
             ('tokens_on_device 2', dict(tokens_on_device=2), (sup, qry, None, None)), ('table_id 4', dict(table_id=4), (sup, qry, None, None)),
             ('table_id -2', dict(table_id=-2), (sup, qry, None, None)),
             ('use_table_lengths without a table', dict(use_table_lengths=1), (sup, qry, None, None)),
             ('use_table_lengths 2', dict(table_id=0, use_table_lengths=2), (sup, qry, None, None)),
             ('lengths with a table', dict(table_id=0), (sup, qry, sl, ql)),
             ('support_len alone', {}, (sup, qry, sl, None)), ('query_len alone', {}, (sup, qry, None, ql)),
             ('no support', {}, (None, qry, None, None)), ('no query', {}, (sup, None, None, None)),
             ('support length max_len + 1', {}, (sup, qry, bad_s, ql)), ('query length 0', {}, (sup, qry, sl, bad_q))]
    for fn, extra in outs.items():
        for what, fields, (s, q, l1, l2) in cases:
            assert raw_call(a, fn, s, q, l1, l2, N, K, Q, extra, **fields) == INVALID, (fn, what)
        for what, nkq in (('N 0', (0, K, Q)), ('K 0', (N, 0, Q)), ('Q 0', (N, K, 0)), ('N < 0', (-1, K, Q))):
            assert raw_call(a, fn, sup, qry, None, None, *nkq, extra) == INVALID, (fn, what)
    assert raw_call(a, 'fsmg_maml_tasks_eval', sup, qry, None, None, N, K, Q, (None, per)) == INVALID          # nowhere to put the NLL
    assert a._lib.fsmg_maml_tasks_step(a._h, None, None, None, None, None, N, K, Q, None, None) == INVALID      # no config
    assert_same_state(state(a), before, 'the refusals')
    assert_same_bits(adapted(a), kept, 'the refusals: the kept theta-prime')                                    # not even an adaptation began
    with pytest.raises(Exception, match='STATE'):
        a.apply_update(1.0)                                      # ... and nothing became pending
    assert raw_call(a, 'fsmg_maml_tasks_step', sup, qry, None, None, N, K, Q, (None, None), inner_steps=n) == 0   # neither loss asked for
    assert a.step == 3 and a.stats()['timeouts'] == 0


@pytest.mark.parametrize('where', ['support', 'query'])
def test_a_bad_token_in_artist_1_skips_the_step(where):
    name = 'B'
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    sup2, qry2 = TR.episode(cfg, (over, N, K, Q, n, seed + 1))
    a, clean = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    assert a.maml_tasks_step(sup, qry, n, LR) == clean.maml_tasks_step(sup, qry, n, LR)
    before = state(a)
    bad_sup, bad_qry = sup.copy(), qry.copy()
    (bad_sup if where == 'support' else bad_qry)[1, 0, 2] = cfg['input_size']             # the start word is no data token
    with pytest.raises(Exception, match='TOKEN_RANGE'):
        a.maml_tasks_step(bad_sup, bad_qry, n, LR)
    assert_same_state(state(a), before, 'the skipped step')
    assert a.stats()['steps_skipped_token_range'] == 1
    with pytest.raises(Exception, match='TOKEN_RANGE'):
        a.maml_tasks_eval(bad_sup, bad_qry, n, LR)
    assert_same_state(state(a), before, 'the refused evaluation')
    assert a.maml_tasks_eval(sup2, qry2, n, LR) == clean.maml_tasks_eval(sup2, qry2, n, LR)
    assert a.maml_tasks_step(sup2, qry2, n, LR) == clean.maml_tasks_step(sup2, qry2, n, LR)
    assert_same_state(state(a), state(clean), 'the next good step')
    assert a.step == 2 and a.stats()['timeouts'] == 0


def test_timed_out_chain_inside_the_step():
    """the handle's own knob (chain_spin_limit 0: the persistent kernels give up at their first wait), as tests/test_maml_paths.py D3:
    the update is skipped on the device, the whole call is repeated once on per-step launches"""
    name = 'D'
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    ref = reference(name, 'tf1_slices')
    a, b = handle(name, shape, cfg, theta), handle(name, shape, cfg, theta)
    a.maml_tasks_eval(sup, qry, n, LR)
    st = a.stats()
    assert st['xcd_launches'] + st['persistent_launches'] > 0 and st['timeouts'] == 0 and st['persistent_path']
    a.debug_set('chain_spin_limit', 0)
    loss, per = a.maml_tasks_step(sup, qry, n, LR, task_loss=True)
    st = a.stats()
    assert st['timeouts'] == 1 and not st['persistent_path'] and st['steps_skipped_timeout'] == 1 and a.step == 1
    assert abs(loss - ref['loss']) <= TR.NLL_RTOL * abs(ref['loss'])
    assert np.all(np.abs(per - ref['task_loss']) <= TR.NLL_RTOL * np.abs(ref['task_loss']))
    b.debug_set('persistent', 0)                                 # what the repeat ran on
    assert np.float32(b.maml_tasks_step(sup, qry, n, LR)) == np.float32(loss)
    assert_same_state(state(a), state(b), 'the repeated step')
    a.debug_set('chain_spin_limit', 1 << 18)
    # ... whose gradient was inside the bounds of T3: the same call on the launches of the repeat, from the same theta
    b.set_params(theta)
    b.maml_tasks_forward_backward(sup, qry, n, LR)
    dist = TR.distance(ref, result(b))
    assert max(dist.values()) <= 1.0, dist
    assert b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- T9
def plugin(cls, cfg, tmp_path, theta, **over):
    m = cls(dict(cfg, checkpt_dir=str(tmp_path), inner_lr=LR, **over))
    m.recover_or_init('')
    m.engine.set_params({k: np.asarray(v, np.float32) for k, v in theta.items()})
    return m


def test_plugin_key(tmp_path):
    from data.episode import Episode
    from models.maml_lstm import MAMLLSTM
    name = 'C'
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    ep = Episode(sup, qry)
    cfg = dict(cfg, name='maml_lstm', inner_steps=n)
    on, ref = (plugin(MAMLLSTM, cfg, tmp_path / d, theta, maml_per_artist=True) for d in ('a', 'b'))
    assert on.maml_per_artist and np.float32(on.eval(ep)) == np.float32(ref.engine.maml_tasks_eval(sup, qry, n, LR))
    on_loss = on.train(ep)
    assert np.float32(on_loss) == np.float32(ref.engine.maml_tasks_step(sup, qry, n, LR))
    assert_same_state(state(on.engine), state(ref.engine), 'train')
    assert on.eval_many([ep, ep]) == [ref.engine.maml_tasks_eval(sup, qry, n, LR)] * 2
    want = TR.reference(MR.f64(theta), sup, qry, cfg, n, LR)['loss']
    assert abs(on_loss - want) <= TR.NLL_RTOL * abs(want)
    off, ref = (plugin(MAMLLSTM, cfg, tmp_path / d, theta) for d in ('c', 'd'))
    assert not off.maml_per_artist and np.float32(off.eval(ep)) == np.float32(ref.engine.maml_eval(sup, qry, n, LR))
    loss = off.train(ep)
    assert np.float32(loss) == np.float32(ref.engine.maml_step(sup, qry, n, LR))                  # today's calls, today's bits
    assert_same_state(state(off.engine), state(ref.engine), 'key off')
    assert np.float32(loss) != np.float32(on_loss)                                                # ... which are another number


def test_meta_sgd_plugin_inherits_the_key(tmp_path):
    from data.episode import Episode
    from models.metasgd_lstm import MetaSGDLSTM
    name = 'C'
    shape, cfg, sup, qry, theta = setup(name)
    over, N, K, Q, n, seed = shape
    ep = Episode(sup, qry)
    cfg = dict(cfg, name='metasgd_lstm', inner_steps=n, alpha_init=0.5, alpha_lr=0.01, alpha_min=0.0, alpha_max=2.0)
    m = plugin(MetaSGDLSTM, cfg, tmp_path, theta, maml_per_artist=True)
    assert m.maml_per_artist and all(np.all(v == np.float32(0.5)) for v in m.rates().values())
    losses = [m.train(ep) for _ in range(2)]
    assert all(np.isfinite(l) and l > 0 for l in losses) and m.engine.step == 2
    rates = m.rates()
    assert any(np.any(v != np.float32(0.5)) for v in rates.values()) and all(np.all((v >= 0) & (v <= 2)) for v in rates.values())
    assert np.isfinite(m.eval(ep))
