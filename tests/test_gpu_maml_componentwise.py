"""-m gpu: the MAML-style pass (cfg-E) against fp64 ELEMENT BY ELEMENT (tests/maml_ref.py has the references and the shapes).

fsmg_debug_set("keep_adapted", 1) makes the handle keep theta' when it puts theta back, fsmg_debug_read("adapted:<name>") reads it.

  C1  theta'_i of every inner step against k_sgd_update's arithmetic redone in fp64 from the DEVICE's own gradient of the support
      pass at theta'_{i-1} (a second handle computes it, the call maml_adapt itself makes), in the derived bound of
      maml_ref.sgd_check; the norm the kernel reports against the norm of those gradients; nothing moves without a gradient.
  C2  every tensor of the query pass against the fp64 oracle at the DEVICE's own theta', in the measures of tests/backward_ref.py
      with the M of tests/test_gpu_componentwise.py: ties every kernel family to the weights the pass should have used -- the
      recurrent-weight images are rebuilt from theta' in between (khf_dirty -> ensure_khf).
  C3  theta'_n, the query loss and the outer gradients against the full fp64 oracle, norm-wise: C1 and C2 start from device
      values, so a consistently wrong gradient could satisfy both.
  C4  fsmg_maml_eval, fsmg_maml_score and fsmg_maml_generate adapt to the same bits as fsmg_maml_forward_backward.

Handles are created for N * (K + Q) sequences, as the plugin does, and run passes of N * K and N * Q rows.
"""
import os

import numpy as np
import pytest

import maml_ref as MR
from gpu_utils import new_model, rel_max
from oracle import lstm_oracle as O
from test_gpu_componentwise import M, check_all, device_tensors

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-4             # the bounds of test_maml_step_and_eval_match_oracle (tests/test_gpu_parity.py)
REL_MAX = 5e-4
LR = MR.INNER_LR


def handle(cfg, theta, shape, mode='tf1_slices', keep=True):
    over, N, K, Q, n, seed = shape
    m = new_model(cfg, theta, max_sequences=N * (K + Q), clip_norm_mode=mode)
    if cfg['hidden_size'] == 512:      # created for > 64 sequences: the bf16-split XCD-local recurrence, whatever the passes' row counts
        forced = os.environ.get('FSMG_XCD_BX3')
        assert bool(m.debug_read('xcd_bx3', 1)[0]) == (N * (K + Q) > 64 if forced is None else forced == '1')
    if keep:
        m.debug_set('keep_adapted', 1)
    return m


def adapted(model):
    return {k: model.get_adapted(k) for k in model.param_shapes}


def assert_same_bits(got, want, what):
    for k in want:
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32)), (what, k)


def assert_format_changes_inside_the_step(model, sup, qry, n):
    """hidden 1024: the support pass alone leaves the bf16-split pair kernels' format, the MAML call the fp32 chains' (its query pass)"""
    N, K = sup.shape[:2]
    model.forward_backward(sup, sup, shape=(N, K, 0))
    assert model.debug_read('xcd_bx3', 1)[0] == 1.0
    model.maml_forward_backward(sup, qry, n, LR)
    assert model.debug_read('xcd_bx3', 1)[0] == 0.0


# ----------------------------------------------------------------------------- C1
C1_CASES = [(i, 'tf1_slices', MR.MAX_GRAD_NORM) for i in range(len(MR.MAML_SHAPES))] + \
           [(1, 'dense', MR.MAX_GRAD_NORM), (3, 'dense', MR.MAX_GRAD_NORM), (1, 'tf1_slices', MR.MAX_GRAD_NORM_INACTIVE)]


@pytest.mark.parametrize('idx,mode,max_grad_norm', C1_CASES, ids=lambda v: str(v))
def test_adapted_parameters_of_every_inner_step_element_by_element(idx, mode, max_grad_norm):
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape, max_grad_norm=max_grad_norm)
    sup, qry = MR.episode(cfg, shape)
    theta = MR.initial_theta(cfg)
    a, b = handle(cfg, theta, shape, mode), handle(cfg, theta, shape, mode, keep=False)
    if cfg['hidden_size'] == 1024:
        assert_format_changes_inside_the_step(a, sup, qry, n)
    with pytest.raises(Exception, match='STATE'):
        b.get_adapted('softmax_b')                               # nothing has been kept on this handle
    label = '%s|%s|%s' % (MR.shape_id(shape), mode, max_grad_norm)
    prev = a.get_params()
    assert_same_bits(prev, theta, 'set_params')
    failures = []
    for i in range(1, n + 1):
        a.maml_forward_backward(sup, qry, i, LR)                 # from the same theta each time: it restores
        got_gnorm = float(a.debug_read('gnorm', 1)[0])           # (the last inner step's; the query pass has no update)
        theta_i = adapted(a)
        assert_same_bits(a.get_params(), theta, 'theta after the call')
        b.set_params(prev)
        b.forward_backward(sup, sup, shape=(N, K, 0))            # the call maml_adapt makes
        grads = {k: b.get_grad(k) for k in b.param_shapes}
        tail = b.debug_read('tail', 16)
        gnorm, step, bad = MR.sgd_check('%s|%d' % (label, i), prev, grads, tail, mode, max_grad_norm, LR, theta_i, got_gnorm)
        failures += ['step %d: %s' % (i, f) for f in bad]
        # the clip is active / inactive as the case says -- the values were chosen from the fp64 oracle's norm (maml_ref.py)
        active = max_grad_norm == MR.MAX_GRAD_NORM
        assert (got_gnorm > max_grad_norm) == active and (gnorm > max_grad_norm) == active, (got_gnorm, gnorm)
        assert (step < float(np.float32(LR))) == active and (active or step == float(np.float32(LR)))
        prev = theta_i
    assert not failures, '%s: %s' % (label, '; '.join(failures))
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- C2
C2_CASES = [(i, 'bx3') for i in range(len(MR.MAML_SHAPES))] + [(1, 'f32'), (4, 'f32')]


@pytest.mark.parametrize('idx,gemm_kind', C2_CASES, ids=lambda v: str(v))
def test_query_pass_at_the_adapted_parameters_element_by_element(idx, gemm_kind, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', gemm_kind)
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape)
    sup, qry = MR.episode(cfg, shape)
    a = handle(cfg, MR.initial_theta(cfg), shape)
    a.debug_set('inplace_dlogits', 0)                            # keep the logits beside dlogits
    if cfg['hidden_size'] == 1024 and gemm_kind == 'bx3':
        assert_format_changes_inside_the_step(a, sup, qry, n)
    a.maml_forward_backward(sup, qry, n, LR)
    assert a.stats()['timeouts'] == 0
    assert a.debug_read('fused_softmax', 2)[1] == 0              # no shape here takes the fused softmax: dlogits is compared
    ref = MR.query_reference(adapted(a), qry, cfg)               # fp64 at the device's own theta'
    got = device_tensors(a, cfg, N * Q)                          # (asserts the pad units of h and c to be exact zeros)
    check_all('maml-%s|%s' % (MR.shape_id(shape), gemm_kind), ref, got)
    loss = float(a.debug_read('tail', 16)[1])
    assert abs(loss - ref.loss) <= NLL_RTOL * abs(ref.loss)


# ----------------------------------------------------------------------------- C3
_ORACLE = {}


def oracle(shape, mode):
    """(theta'_n, query loss, outer gradients, inner steps) of the fp64 oracle: computed once per (shape, mode), never written to"""
    key = (MR.shape_id(shape), mode)
    if key not in _ORACLE:
        over, N, K, Q, n, seed = shape
        cfg = MR.config_of(shape)
        sup, qry = MR.episode(cfg, shape)
        p64 = MR.f64(MR.initial_theta(cfg))
        fast, _ = O.maml_adapt(p64, sup, cfg, n, LR, clip_norm_mode=mode)
        loss, grads, _ = O.maml_query_grads(p64, sup, qry, cfg, n, LR, clip_norm_mode=mode)
        _, steps = MR.adapt_full(p64, sup, cfg, n, LR, mode)
        _ORACLE[key] = (fast, loss, grads, steps)
    return _ORACLE[key]


@pytest.mark.parametrize('mode', ['tf1_slices', 'dense'])
@pytest.mark.parametrize('idx', range(len(MR.MAML_SHAPES)))
def test_adapted_parameters_and_outer_gradients_match_the_oracle(idx, mode):
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape)
    sup, qry = MR.episode(cfg, shape)
    want_theta, want_loss, want_grads, steps = oracle(shape, mode)
    a = handle(cfg, MR.initial_theta(cfg), shape, mode)
    a.maml_forward_backward(sup, qry, n, LR)
    assert a.stats()['timeouts'] == 0
    got_theta = adapted(a)
    loss = float(a.debug_read('tail', 16)[1])
    assert abs(loss - want_loss) <= NLL_RTOL * abs(want_loss), (loss, want_loss)
    for k in want_theta:
        assert rel_max(got_theta[k], want_theta[k]) < REL_MAX, ('theta', k)
        assert rel_max(a.get_grad(k), want_grads[k]) < REL_MAX, ('gradient', k)
    # The clip is active in every inner step here, so the two modes' theta' differ -- but by 0.03 % of the step (the norms differ in
    # their fourth digit, maml_ref.py), which is inside REL_MAX for every tensor but the biases: this comparison cannot tell the
    # modes apart.  C1's bound can: in every tensor the two oracles are far more than 10 bounds apart.
    other = oracle(shape, 'dense' if mode == 'tf1_slices' else 'tf1_slices')
    assert all(s['gnorm'] > cfg['max_grad_norm'] for s in steps + other[3])
    for k in want_theta:
        p_ref, sg = MR.sgd_reference(steps[-1]['before'][k], steps[-1]['grads'][k], steps[-1]['gnorm'], cfg['max_grad_norm'], LR)
        tol = 2 * MR.U * np.abs(p_ref) + 8 * MR.U * sg + 1e-30
        apart = float((np.abs(want_theta[k] - other[0][k]) / tol).max())
        print('MODES|%s|%s|%.0f bounds apart, rel_max %.1e' % (MR.shape_id(shape), k, apart, rel_max(other[0][k], want_theta[k])))
        assert apart > 10, k


# ----------------------------------------------------------------------------- C4
@pytest.mark.parametrize('idx', [1, 3])
def test_eval_score_and_generate_adapt_to_the_same_bits(idx):
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape)
    sup, qry = MR.episode(cfg, shape)
    theta = MR.initial_theta(cfg)
    a = handle(cfg, theta, shape)
    a.maml_forward_backward(sup, qry, n, LR)
    want = adapted(a)
    assert max(rel_max(want[k], theta[k]) for k in want if not k.startswith('bias_')) > 1e-3          # it is theta', not theta
    flat = sup.reshape(N * K, cfg['max_len'])                    # with_adapted_theta adapts on N = 1, K = rows
    calls = [('maml_eval', lambda m: m.maml_eval(sup, qry, n, LR)),
             ('maml_score', lambda m: m.maml_score(flat, qry.reshape(N * Q, cfg['max_len']), n, LR)),
             ('maml_generate', lambda m: m.maml_generate(flat, 4, n, LR, n_seq=2, seed=1))]
    for name, call in calls:
        m = handle(cfg, theta, shape)
        call(m)
        assert_same_bits(adapted(m), want, name)
        assert_same_bits(m.get_params(), theta, name + ': theta afterwards')
        assert m.stats()['timeouts'] == 0
        call(a)                                                  # ... and on the handle that has run the train form before
        assert_same_bits(adapted(a), want, name + ' after maml_forward_backward')
        assert_same_bits(a.get_params(), theta, name + ': theta afterwards')
    assert a.stats()['timeouts'] == 0
