"""-m gpu: Meta-SGD, the learned per-parameter inner rates of the MAML-style step (include/fsmg.h "Meta-SGD", DESIGN.md 24;
references and bounds in tests/msgd_ref.py, measured figures in tests/COMPONENTWISE_MSGD.md).

  L1 .. L8  bitwise laws between two handles or two runs
  E1        theta'_i of every inner step, S and GA against fp64 from the DEVICE's own gradients, element by element
  E2        A, AM, AV after the update against fp64 from the device's own GA (one case with both clamp ends binding)
  F1        three outer steps and maml_eval against msgd_ref in fp64
  P1        the plugin on the golden lyrics;  R1  refusals through the C ABI
"""
import os

import numpy as np
import pytest

import maml_ref as MR
import msgd_ref as SR
from gpu_utils import new_model, rel_max
from oracle import lstm_oracle as O
from test_gpu_maml_componentwise import NLL_RTOL, REL_MAX, adapted, assert_same_bits
from test_maml_paths import assert_same_state, state

pytestmark = pytest.mark.gpu

LR = MR.INNER_LR
ALL = range(len(MR.MAML_SHAPES))


def handle(cfg, theta, shape, mode='tf1_slices', rates=None, **mcfg):
    """rates: None = never enabled; a float = enabled and filled; a dict = enabled and set per tensor"""
    over, N, K, Q, n, seed = shape
    m = new_model(cfg, theta, max_sequences=N * (K + Q), clip_norm_mode=mode)
    m.debug_set('keep_adapted', 1)
    if rates is not None:
        m.msgd_enable(**SR.msgd_config(**mcfg))
        if isinstance(rates, dict):
            for k, v in rates.items():
                m.msgd_set_alpha(k, v)
        else:
            m.msgd_fill(rates)
    return m


def case(idx, **over):
    shape = MR.MAML_SHAPES[idx]
    cfg = MR.config_of(shape, **over)
    sup, qry = MR.episode(cfg, shape)
    return shape, cfg, sup.astype(np.int32), qry.astype(np.int32), MR.initial_theta(cfg)


def rate_state(m):
    return {k: (m.msgd_get_alpha(k),) + m.msgd_get_opt_state(k) for k in m.param_shapes}


def same_rate_state(a, b, what=''):
    for k in a:
        for i, name in enumerate(('A', 'AM', 'AV')):
            assert np.array_equal(a[k][i].view(np.uint32), b[k][i].view(np.uint32)), (what, name, k)


def sums(m):
    return {k: m.msgd_get_sum(k) for k in m.param_shapes}


def rate_grads(m):
    return {k: m.msgd_get_grad(k) for k in m.param_shapes}


def table_of(sup, qry):
    N, K, T = sup.shape
    Q = qry.shape[1]
    table = np.concatenate([sup.reshape(N * K, T), qry.reshape(N * Q, T)])
    return table, np.arange(N * K, dtype=np.int32).reshape(N, K), (N * K + np.arange(N * Q, dtype=np.int32)).reshape(N, Q)


# ----------------------------------------------------------------------------- L1
@pytest.mark.parametrize('idx', ALL)
def test_unit_rates_are_the_plain_step_bit_for_bit(idx):
    """enabled with A == 1 and alpha_lr == 0 against a never-enabled twin: st = step * 1 is exact and the element line is
    k_sgd_update's, so everything agrees bit for bit"""
    shape, cfg, sup, qry, theta = case(idx)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    a, b = handle(cfg, theta, shape, rates=1.0, alpha_lr=0.0), handle(cfg, theta, shape)
    assert a.msgd_info() == dict(enabled=True, allocated=True, count=a.msgd_info()['count'], pending=False)
    assert b.msgd_info()['enabled'] is False and b.msgd_info()['allocated'] is False
    table, si, qi = table_of(sup, qry)
    fs, fq = np.full((N, K), T, np.int32), np.full((N, Q), T, np.int32)
    for m in (a, b):
        m.upload_table(0, table)
    steps = [('plain', lambda m: m.maml_step(sup, qry, n, LR)),
             ('masked', lambda m: m.maml_step_masked(sup, qry, fs, fq, n, LR)),
             ('indexed', lambda m: m.maml_step_indexed(0, si, qi, n, LR))]
    for name, call in steps:
        la, lb = call(a), call(b)
        assert np.float32(la) == np.float32(lb), name
        assert_same_state(state(a), state(b), name)
        assert_same_bits(adapted(a), adapted(b), name + ': theta-prime')
    flat, qflat = sup.reshape(N * K, T), qry.reshape(N * Q, T)
    assert np.float32(a.maml_eval(sup, qry, n, LR)) == np.float32(b.maml_eval(sup, qry, n, LR))
    sa, sb = a.maml_score(flat, qflat, n, LR), b.maml_score(flat, qflat, n, LR)
    for k in sb:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), ('maml_score', k)
    assert np.array_equal(a.maml_generate(flat, 4, n, LR, n_seq=2, seed=1), b.maml_generate(flat, 4, n, LR, n_seq=2, seed=1))
    assert_same_state(state(a), state(b), 'after the forward-only calls')
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0 and a.step == 3


# ----------------------------------------------------------------------------- L2
@pytest.mark.parametrize('idx', [1, 3])
def test_rate_two_at_x_is_rate_one_at_two_x(idx):
    shape, cfg, sup, qry, theta = case(idx)
    n = shape[4]
    a, b = handle(cfg, theta, shape, rates=2.0), handle(cfg, theta, shape, rates=1.0)
    a.maml_forward_backward(sup, qry, n, 0.05)
    b.maml_forward_backward(sup, qry, n, 0.1)
    assert_same_bits(adapted(a), adapted(b), 'theta-prime')
    Sa, Sb, Ga, Gb = sums(a), sums(b), rate_grads(a), rate_grads(b)
    for k in Sa:
        assert np.array_equal((2 * Sa[k]).view(np.uint32), Sb[k].view(np.uint32)), ('S', k)
        assert np.array_equal(2 * Ga[k], Gb[k]), ('GA', k)
        assert np.any(Sa[k] != 0) and np.any(Ga[k] != 0), k


# ----------------------------------------------------------------------------- L3, L4, L6
@pytest.mark.parametrize('idx', [1, 3])
def test_disable_reenable_untouched_rates_and_two_runs(idx):
    shape, cfg, sup, qry, theta = case(idx)
    over, N, K, Q, n, seed = shape
    T = cfg['max_len']
    A = SR.draw_rates(cfg)
    flat, qflat = sup.reshape(N * K, T), qry.reshape(N * Q, T)

    def run():
        m = handle(cfg, theta, shape, rates=A)
        losses = [m.maml_step(sup, qry, n, LR) for _ in range(2)]
        return m, losses, state(m), rate_state(m), adapted(m)
    a, la, sa, ra, ta = run()
    b, lb, sb, rb, tb = run()
    assert [np.float32(x) for x in la] == [np.float32(x) for x in lb]                     # L6
    assert_same_state(sa, sb, 'two runs')
    same_rate_state(ra, rb, 'two runs')
    assert_same_bits(ta, tb, 'two runs: theta-prime')
    assert any(np.any(ra[k][0] != A[k]) for k in A)                                       # (the rates moved: alpha_lr > 0)
    # L4: forward-only calls leave A and its slots alone; so does a step with alpha_lr == 0
    a.maml_eval(sup, qry, n, LR)
    a.maml_score(flat, qflat, n, LR)
    a.maml_generate(flat, 4, n, LR, n_seq=2, seed=1)
    same_rate_state(rate_state(a), ra, 'eval / score / generate')
    a.msgd_enable(**SR.msgd_config(alpha_lr=0.0))
    a.maml_step(sup, qry, n, LR)
    same_rate_state(rate_state(a), ra, 'alpha_lr == 0')
    assert a.step == 3
    # L3: disabled, the step is a never-enabled handle's; re-enabling finds the state
    c = handle(cfg, theta, shape)
    c.set_params(a.get_params())
    for k in c.param_shapes:
        c.set_opt_state(k, *a.get_opt_state(k))
    c.step = a.step
    a.msgd_disable()
    assert np.float32(a.maml_step(sup, qry, n, LR)) == np.float32(c.maml_step(sup, qry, n, LR))
    assert_same_state(state(a), state(c), 'disabled')
    assert_same_bits(adapted(a), adapted(c), 'disabled: theta-prime')
    a.msgd_enable(**SR.msgd_config())
    same_rate_state(rate_state(a), ra, 're-enabled')
    assert a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- L5
def test_without_inner_steps_nothing_is_collected():
    shape, cfg, sup, qry, theta = case(1)
    A = SR.draw_rates(cfg)
    a = handle(cfg, theta, shape, rates=A)
    a.maml_forward_backward(sup, qry, 1, LR)                       # leave something in S and GA first
    a.maml_forward_backward(sup, qry, 0, LR)
    assert a.msgd_info()['pending']
    for k in A:
        assert np.all(a.msgd_get_sum(k) == 0) and np.all(a.msgd_get_grad(k) == 0), k
    a.apply_update(1.0)
    assert not a.msgd_info()['pending']
    with pytest.raises(Exception, match='STATE'):
        a.msgd_get_grad('softmax_b')
    for k in A:
        assert np.array_equal(a.msgd_get_alpha(k).view(np.uint32), A[k].view(np.uint32)), k
    assert a.step == 1


# ----------------------------------------------------------------------------- L7
@pytest.mark.parametrize('idx', [0, 3])
def test_masked_against_unmasked_with_nonuniform_rates(idx):
    """tests/test_gpu_maml_masked.py's laws with rates that differ per element: full lengths are the unmasked call bit for bit; what
    stands behind a song's end never matters"""
    from test_gpu_maml_masked import case as masked_case, scrambled
    shape, cfg, sup, qry, sl, ql = masked_case(idx)
    n, T = shape[4], cfg['max_len']
    theta, A = MR.initial_theta(cfg), SR.draw_rates(cfg)
    fs, fq = np.full_like(sl, T), np.full_like(ql, T)

    def everything(call):
        m = handle(cfg, theta, shape, rates=A)
        call(m)
        out = dict(theta=adapted(m), S=sums(m), GA=rate_grads(m), G={k: m.get_grad(k) for k in m.param_shapes})
        out['loss'] = np.float32(m.apply_update(1.0))
        out['state'], out['rates'] = state(m), rate_state(m)
        assert m.stats()['timeouts'] == 0
        return out

    def same(x, y, what):
        for key in ('theta', 'S', 'GA', 'G'):
            assert_same_bits(x[key], y[key], what + ': ' + key)
        assert x['loss'] == y['loss'], what
        assert_same_state(x['state'], y['state'], what)
        same_rate_state(x['rates'], y['rates'], what)
    u = everything(lambda m: m.maml_forward_backward(sup, qry, n, LR))
    f = everything(lambda m: m.maml_forward_backward_masked(sup, qry, fs, fq, n, LR))
    same(u, f, 'full lengths')
    sup2, qry2 = scrambled(cfg, sup, qry, sl, ql)
    p = everything(lambda m: m.maml_forward_backward_masked(sup, qry, sl, ql, n, LR))
    q = everything(lambda m: m.maml_forward_backward_masked(sup2, qry2, sl, ql, n, LR))
    same(p, q, 'padding')
    assert p['loss'] != u['loss'] and not np.array_equal(p['GA']['softmax_w'], u['GA']['softmax_w'])


# ----------------------------------------------------------------------------- L8
def test_timed_out_chain_inside_the_step_moves_the_rates_once():
    """the spin limit forced to 0 (tests/test_maml_paths.py's knob): the step is skipped on the device and repeated once on per-step
    launches -- S, GA, A and theta are those of a handle on per-step launches from the start, and A moved once"""
    shape, cfg, sup, qry, theta = case(3)
    n = shape[4]
    A = SR.draw_rates(cfg)
    a, b = handle(cfg, theta, shape, rates=A), handle(cfg, theta, shape, rates=A)
    st = a.stats()
    b.debug_set('persistent', 0)
    a.debug_set('chain_spin_limit', 0)
    la, lb = a.maml_step(sup, qry, n, LR), b.maml_step(sup, qry, n, LR)
    st = a.stats()
    assert st['timeouts'] == 1 and not st['persistent_path'] and st['steps_skipped_timeout'] == 1 and b.stats()['timeouts'] == 0
    assert np.float32(la) == np.float32(lb)
    assert_same_state(state(a), state(b), 'recovered step')
    same_rate_state(rate_state(a), rate_state(b), 'recovered step')
    assert_same_bits(sums(a), sums(b), 'S')
    assert_same_bits(adapted(a), adapted(b), 'theta-prime')
    assert a.step == 1
    # A moved once: one Adam step from zero slots leaves AM = (1 - b1) * GA * scale, not twice that
    c = handle(cfg, theta, shape, rates=A)
    c.debug_set('persistent', 0)
    c.maml_forward_backward(sup, qry, n, LR)
    GA = rate_grads(c)
    for k in GA:
        m1 = a.msgd_get_opt_state(k)[0]
        want = float(np.float32(1.0) - np.float32(0.9)) * GA[k].astype(np.float64)
        assert np.all(np.abs(m1 - want) <= 16 * SR.U * np.abs(want) + SR.UNDERFLOW), k


# ----------------------------------------------------------------------------- E1
E1_CASES = [(i, 'tf1_slices') for i in ALL] + [(1, 'dense'), (3, 'dense')]


@pytest.mark.parametrize('idx,mode', E1_CASES, ids=str)
def test_inner_steps_sum_and_rate_gradient_element_by_element(idx, mode):
    """the method of tests/test_gpu_maml_componentwise.py C1: the support gradient at theta'_{i-1} is re-obtained on a second handle by
    the call maml_adapt itself makes, and k_msgd_update / k_msgd_alpha_grad are redone from it in fp64 (msgd_ref.theta_check,
    sum_reference, ga_reference)"""
    shape, cfg, sup, qry, theta = case(idx)
    over, N, K, Q, n, seed = shape
    A = SR.draw_rates(cfg)
    a, b = handle(cfg, theta, shape, mode, rates=A), handle(cfg, theta, shape, mode)
    label = '%s|%s' % (MR.shape_id(shape), mode)
    prev, failures, step_grads = a.get_params(), [], []
    for i in range(1, n + 1):
        a.maml_forward_backward(sup, qry, i, LR)
        got_gnorm = float(a.debug_read('gnorm', 1)[0])
        theta_i = adapted(a)
        assert_same_bits(a.get_params(), theta, 'theta after the call')
        b.set_params(prev)
        b.forward_backward(sup, sup, shape=(N, K, 0))
        grads = {k: b.get_grad(k) for k in b.param_shapes}
        tail = b.debug_read('tail', 16)
        gnorm, step, bad = SR.theta_check('%s|%d' % (label, i), prev, A, grads, tail, mode, cfg['max_grad_norm'], LR, theta_i, got_gnorm)
        assert gnorm > cfg['max_grad_norm'] and step < float(np.float32(LR))              # the clip is active
        failures += ['step %d: %s' % (i, f) for f in bad]
        step_grads.append((step, grads))
        prev = theta_i
    S, GA, G = sums(a), rate_grads(a), {k: a.get_grad(k) for k in a.param_shapes}
    S_ref, S_tol = SR.sum_reference(step_grads)
    GA_ref, GA_tol = SR.ga_reference(G, S)
    for k in sorted(S):
        fs = np.abs(S[k] - S_ref[k]) / S_tol[k]
        fg = np.abs(GA[k] - GA_ref[k]) / GA_tol[k]
        print('MSGD|S|%s|%s|%.3f|GA %.3f' % (label, k, fs.max(), fg.max()))
        if (fs > 1).any():
            failures.append('S %s: worst %.1f x' % (k, fs.max()))
        if (fg > 1).any():
            failures.append('GA %s: worst %.1f x' % (k, fg.max()))
        if not np.all(S[k][np.all([g[k] == 0 for _, g in step_grads], axis=0)] == 0):
            failures.append('S %s: an element without a gradient is not zero' % k)
    assert not failures, '%s: %s' % (label, '; '.join(failures))
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- E2
E2_CASES = [(1, 0.0, 10.0, 0.0), (3, 0.0, 10.0, 1e-3), (1, 0.9, 1.1, 0.0)]      # (shape, alpha_min, alpha_max, alpha_clip_norm); last: both ends bind


@pytest.mark.parametrize('idx,lo,hi,clip', E2_CASES, ids=str)
def test_rates_update_element_by_element(idx, lo, hi, clip):
    shape, cfg, sup, qry, theta = case(idx)
    n = shape[4]
    A = SR.draw_rates(cfg)
    mcfg = SR.msgd_config(alpha_min=lo, alpha_max=hi, alpha_clip_norm=clip)
    a = handle(cfg, theta, shape, rates=A, **mcfg)
    failures = []
    for s in range(2):                                             # the second step exercises b1 * m and b2 * v
        a.maml_forward_backward(sup, qry, n, LR)
        GA = rate_grads(a)
        A0, slots0 = {k: a.msgd_get_alpha(k) for k in A}, {k: a.msgd_get_opt_state(k) for k in A}
        gnorm, scale, size = SR.alpha_scalars(GA, s, dict(cfg, lr=float(np.float32(cfg['lr'])), n_decay=float(np.float32(cfg['n_decay']))),
                                              {k: float(np.float32(v)) for k, v in mcfg.items()})
        assert (clip > 0) == (scale < 1.0), (gnorm, scale)          # the rates' clip is active where the case sets one
        a.apply_update(1.0)
        assert a.step == s + 1
        A1, slots1 = {k: a.msgd_get_alpha(k) for k in A}, {k: a.msgd_get_opt_state(k) for k in A}
        failures += SR.alpha_check('%s|%s|%s|step %d' % (MR.shape_id(shape), lo, clip, s), A0, slots0, GA, A1, slots1, scale, size,
                                   float(np.float32(lo)), float(np.float32(hi)))
        if lo > 0 and s == 0:
            assert any(np.any(A1[k] == np.float32(lo)) for k in A) and any(np.any(A1[k] == np.float32(hi)) for k in A)
            assert all(np.all((A1[k] >= np.float32(lo)) & (A1[k] <= np.float32(hi))) for k in A)
    assert not failures, '; '.join(failures)


# ----------------------------------------------------------------------------- F1
@pytest.mark.parametrize('idx', ALL)
def test_three_outer_steps_and_eval_match_fp64(idx):
    """losses and the NLL to the project's 1e-4 relative; theta and A per tensor by rel_max < 5e-4, the measure and bound the MAML tests
    use after outer updates (tests/test_gpu_parity.py test_maml_step_and_eval_match_oracle, REL_MAX of the component-wise file)"""
    shape, cfg, sup, qry, theta = case(idx)
    over, N, K, Q, n, seed = shape
    mcfg = SR.msgd_config()
    A32 = SR.draw_rates(cfg)
    a = handle(cfg, theta, shape, rates=A32, **mcfg)
    params, A = MR.f64(theta), MR.f64(A32)
    opt, st = O.new_opt_state(params), SR.new_rate_state(A)
    eps = [MR.R.episode(cfg, N, K, Q, seed + s) for s in range(4)]
    for s in range(3):
        want, _ = SR.msgd_step(params, opt, A, st, eps[s][0], eps[s][1], cfg, mcfg, n, LR)
        got = a.maml_step(eps[s][0], eps[s][1], n, LR)
        print('MSGD|e2e|%s|step %d|loss %.3e' % (MR.shape_id(shape), s, abs(got - want) / abs(want)))
        assert abs(got - want) <= NLL_RTOL * abs(want), (s, got, want)
    want = SR.msgd_eval(params, A, eps[3][0], eps[3][1], cfg, n, LR)
    got = a.maml_eval(eps[3][0], eps[3][1], n, LR)
    assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
    plain = O.maml_eval(params, eps[3][0], eps[3][1], cfg, n, LR)
    assert abs(want - plain) > 2 * NLL_RTOL * abs(plain)           # the rates move the NLL by more than the bound is wide: the check has teeth
    worst = {}
    for k in params:
        worst[k] = (rel_max(a.get_param(k), params[k]), rel_max(a.msgd_get_alpha(k), A[k]))
        print('MSGD|e2e|%s|%s|theta %.2e|A %.2e' % (MR.shape_id(shape), k, worst[k][0], worst[k][1]))
    assert a.step == 3 and a.stats()['timeouts'] == 0
    for k, (t, r) in worst.items():
        assert t < REL_MAX, ('theta', k, t)
        assert r < REL_MAX, ('A', k, r)


# ----------------------------------------------------------------------------- P1
def test_plugin_on_the_golden_lyrics(tmp_path, golden_dir):
    import yaml
    from conftest import ROOT
    from data.episode import load_sampler_from_config
    from models.metasgd_lstm import MetaSGDLSTM
    from test_masked_cpu import K, Q, T, _dataset, _raw_tree
    from test_train_entry import LOOP
    shipped = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'metasgd_lstm.yaml')))
    assert shipped['model_class_name'] == 'MetaSGDLSTM' and shipped['alpha_init'] == 1.0
    root = _raw_tree(tmp_path, golden_dir)
    _dataset(root)[0].metadata.close()
    full = dict(LOOP, name='metasgd_lstm', model_module_name=shipped['model_module_name'], model_class_name=shipped['model_class_name'],
                n_decay=10000, lr=5e-3, max_grad_norm=5, embedding_size=32, hidden_size=40, n_layers=1, dataset='lyrics', dataset_path=root,
                splits=['train', 'val', 'test'], max_len=T, query_size=Q, support_size=K, seed=1234, split='train',
                inner_steps=1, inner_lr=0.3, alpha_init=0.5, alpha_lr=0.01, alpha_min=0.0, alpha_max=2.0)
    sampler = load_sampler_from_config(dict(full))
    full['input_size'] = sampler.get_num_unique_words()
    eps = [sampler.get_episode() for _ in range(4)]
    model = MetaSGDLSTM(dict(full))
    model.recover_or_init('')
    assert all(np.all(v == np.float32(0.5)) for v in model.rates().values())
    losses = [model.train(e) for e in eps[:3]]
    assert all(np.isfinite(l) and l > 0 for l in losses)
    nll = model.eval(eps[3])
    assert np.isfinite(nll) and nll > 0
    sup = np.asarray(eps[3].support)
    flat = sup.reshape(-1, sup.shape[-1])
    toks = model.generate(flat, 5, n=2, seed=3)
    assert np.asarray(toks).shape == (2, 5)
    sc = model.score(flat, np.asarray(eps[3].query).reshape(-1, sup.shape[-1]))
    assert np.all(np.isfinite(sc['row_nll']))
    rates = model.rates()
    assert any(np.any(v != np.float32(0.5)) for v in rates.values())           # moved from alpha_init
    assert all(np.all((v >= 0) & (v <= 2)) for v in rates.values())
    before = rate_state(model.engine)
    model.save(str(tmp_path / 'ck'))
    again = MetaSGDLSTM(dict(full))
    again.recover_or_init(str(tmp_path / 'ck'))
    same_rate_state(rate_state(again.engine), before, 'save / recover')
    assert again.engine.step == 3
    assert np.float32(again.eval(eps[3])) == np.float32(nll)


# ----------------------------------------------------------------------------- R1
def test_refusals_through_the_c_abi():
    import ctypes as C
    from fsmg.binding import FsmgMsgdConfig
    shape, cfg, sup, qry, theta = case(0)
    m = handle(cfg, theta, shape)
    for call in (lambda: m.msgd_fill(1.0), lambda: m.msgd_get_alpha('softmax_b'), lambda: m.msgd_grad_buffer(),
                 lambda: m.msgd_get_sum('softmax_b')):
        with pytest.raises(Exception, match='STATE'):
            call()
    nan, inf = float('nan'), float('inf')
    bad = [dict(alpha_lr=-1.0), dict(alpha_lr=inf), dict(alpha_lr=nan), dict(alpha_clip_norm=-1.0), dict(alpha_clip_norm=inf),
           dict(alpha_clip_norm=nan), dict(alpha_min=2.0, alpha_max=1.0), dict(alpha_min=nan), dict(alpha_max=nan), dict(alpha_init=nan),
           dict(alpha_init=inf)]
    for kw in bad:
        with pytest.raises(Exception, match='INVALID'):
            m.msgd_enable(**SR.msgd_config(**kw))
    for field, value in (('struct_size', 4), ('reserved', 1)):
        c = m.msgd_config(**SR.msgd_config())
        setattr(c, field, value)
        with pytest.raises(Exception, match='INVALID'):
            m.msgd_enable(c)
    assert m.msgd_info()['allocated'] is False                     # every refusal came before any device work
    m.msgd_enable(**SR.msgd_config())
    with pytest.raises(Exception, match='INVALID'):
        m.msgd_set_alpha('softmax_b', np.full(m._shape('softmax_b'), inf, np.float32))
    with pytest.raises(Exception, match='INVALID'):
        m.msgd_fill(nan)
    with pytest.raises(Exception, match='SIZE'):
        m.msgd_set_alpha('softmax_b', np.ones(3, np.float32))
    with pytest.raises(Exception, match='NAME'):
        m.msgd_get_alpha('no_such_tensor')
    with pytest.raises(Exception, match='STATE'):
        m.msgd_get_grad('softmax_b')                               # nothing pending


def test_a_library_communicator_and_the_rates_exclude_each_other():
    """one rank on one GPU, as tests/test_dist_hip.py has it"""
    from fsmg.binding import FsmgModel
    shape, cfg, sup, qry, theta = case(0)
    m = handle(cfg, theta, shape, rates=1.0)
    uid = FsmgModel.comm_unique_id()
    with pytest.raises(Exception, match='STATE'):
        m.comm_init(uid, 1, 0)
    m.msgd_disable()
    m.comm_init(uid, 1, 0)
    with pytest.raises(Exception, match='STATE'):
        m.msgd_enable(**SR.msgd_config())
    assert m.msgd_info()['enabled'] is False
