"""The checks of tests/test_gpu_maml_componentwise.py on the CPU alone: the restatement is the oracle, the fp32 stand-in of the device
(maml_ref.standin_update: k_sgd_update in numpy fp32; the oracle's fp32 pass for the query rows) passes C1's bound and C2's M * e32,
and the same stand-in with one planted mistake does not -- the checks have teeth.  What is tested here is the checks, not a kernel.
"""
import numpy as np
import pytest

import maml_ref as MR
from oracle import lstm_oracle as O

M = 8                        # tests/test_gpu_componentwise.py
NLL_RTOL = 1e-4              # the loss bound of the norm-wise MAML tests (tests/test_gpu_parity.py)
LR = MR.INNER_LR
SHAPES = list(range(len(MR.MAML_SHAPES)))            # the hidden-1024 shape takes 2 s here: all of them


def setup(idx, **over):
    shape = MR.MAML_SHAPES[idx]
    cfg = MR.config_of(shape, **over)
    sup, qry = MR.episode(cfg, shape)
    return shape, cfg, sup, qry, MR.initial_theta(cfg)


@pytest.mark.parametrize('mode', ['tf1_slices', 'dense'])
@pytest.mark.parametrize('idx', [0, 1, 2])
def test_restatement_is_the_oracle_bit_for_bit(idx, mode):
    shape, cfg, sup, qry, theta = setup(idx)
    n = shape[4] + 1                                  # one step more than the shape runs: every shape has a second step here
    p64 = MR.f64(theta)
    want, want_losses = O.maml_adapt(p64, sup, cfg, n, LR, clip_norm_mode=mode)
    got, steps = MR.adapt_full(p64, sup, cfg, n, LR, mode)
    assert [s['loss'] for s in steps] == want_losses and len(steps) == n
    for k in want:
        assert got[k].dtype == np.float64
        np.testing.assert_array_equal(got[k], want[k])
        np.testing.assert_array_equal(steps[-1]['theta'][k], want[k])
        np.testing.assert_array_equal(steps[0]['before'][k], p64[k])
    for i in range(1, n):                             # step i + 1 starts from theta'_i
        for k in want:
            np.testing.assert_array_equal(steps[i]['before'][k], steps[i - 1]['theta'][k])
    # its first step is the plain pass over the support rows alone, the call the library's maml_adapt makes
    X, Y = O.train_xy(sup, sup[:, :0], cfg['input_size'])
    _, cache = O.forward(p64, X, Y, cfg)
    grads, aux = O.backward(p64, cache, cfg)
    for k in grads:
        np.testing.assert_array_equal(steps[0]['grads'][k], grads[k])
    assert steps[0]['gnorm'] == O.global_norm(grads, aux, mode)


def test_device_gnorm_and_step_restate_the_kernel():
    shape, cfg, sup, qry, theta = setup(1)
    _, steps = MR.adapt_full(theta, sup, cfg, 1, LR)
    g, aux = steps[0]['grads'], steps[0]['aux']
    tail = MR.standin_tail(aux)
    dense = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
    assert MR.device_gnorm(g, tail, 'dense') == dense
    slices = np.sqrt(dense ** 2 - float((g['embedding'].astype(np.float64) ** 2).sum()) + float(tail[0]))
    assert abs(MR.device_gnorm(g, tail, 'tf1_slices') - slices) <= 1e-12 * slices and slices != dense
    # fp32 constants: 0.3 and 0.1 are not fp32 numbers
    clip, lr = float(np.float32(0.3)), np.float32(0.1)
    assert MR.sgd_step(dense, 0.3, 0.1) == float(np.float32(clip / dense) * lr) and dense > clip
    assert MR.sgd_step(dense, 50, 0.1) == float(lr)
    p_ref, sg = MR.sgd_reference(theta['softmax_b'], g['softmax_b'], dense, 0.3, 0.1)
    assert p_ref.dtype == np.float64 and np.all(sg == np.abs(MR.sgd_step(dense, 0.3, 0.1) * g['softmax_b'].astype(np.float64)))


@pytest.mark.parametrize('mode,max_grad_norm', [('tf1_slices', MR.MAX_GRAD_NORM), ('dense', MR.MAX_GRAD_NORM),
                                                ('tf1_slices', MR.MAX_GRAD_NORM_INACTIVE)])
@pytest.mark.parametrize('idx', SHAPES)
def test_fp32_stand_in_passes_both_checks(idx, mode, max_grad_norm):
    shape, cfg, sup, qry, theta = setup(idx, max_grad_norm=max_grad_norm)
    n = shape[4]
    fast, failures = MR.adapt_failures(MR.shape_id(shape), theta, sup, cfg, n, LR, mode)
    assert not failures, failures
    # the clip is active / inactive as the GPU cases say: from the fp64 oracle's norm
    _, steps = MR.adapt_full(MR.f64(theta), sup, cfg, n, LR, mode)
    assert all((s['gnorm'] > max_grad_norm) == (max_grad_norm == MR.MAX_GRAD_NORM) for s in steps), [s['gnorm'] for s in steps]
    ref = MR.query_reference(fast, qry, cfg)
    loss, got = MR.pass_tensors32(fast, qry, cfg)
    assert MR.query_failures(ref, got, M) == {}
    assert abs(loss - ref.loss) <= NLL_RTOL * abs(ref.loss)


# ----------------------------------------------------------------------------- the checks have teeth
# which planted mistake fails on which shape (index into MAML_SHAPES).  dense_norm and no_clip need an active clip: every shape at
# MAX_GRAD_NORM; the others do not care
CAUGHT_BY_C1 = {'dense_norm': SHAPES, 'no_clip': SHAPES, 'last_float4': SHAPES, 'absent_row_ulp': SHAPES}


@pytest.mark.parametrize('wrong', MR.WRONG)
def test_a_planted_mistake_in_the_update_fails_the_elementwise_check(wrong):
    for idx in CAUGHT_BY_C1[wrong]:
        shape, cfg, sup, qry, theta = setup(idx)
        _, failures = MR.adapt_failures(MR.shape_id(shape), theta, sup, cfg, shape[4], LR, 'tf1_slices', wrong)
        print('TEETH|%s|%s|%s' % (wrong, MR.shape_id(shape), failures))
        assert failures, (wrong, MR.shape_id(shape))
        what = ' '.join(failures)
        if wrong == 'dense_norm':                     # the reported norm AND the elements (the scale that came from it)
            assert 'gnorm' in what and 'outside the bound' in what
        elif wrong == 'no_clip':
            assert 'gnorm' not in what and 'outside the bound' in what
        elif wrong == 'last_float4':                  # exactly the four elements, nothing else
            assert len(failures) == shape[4] and all(f.split(': ')[1] == 'softmax_b' and ': 4 of' in f for f in failures)
        else:
            assert all('embedding: 1 elements without a gradient moved' in f for f in failures) and 'outside' not in what


def test_the_inactive_clip_hides_a_wrong_norm_from_theta_but_not_from_the_norm_check():
    """why the GPU cases run with the clip active: with max_grad_norm above the norm the scale is 1 whatever the norm was"""
    shape, cfg, sup, qry, theta = setup(1, max_grad_norm=MR.MAX_GRAD_NORM_INACTIVE)
    _, failures = MR.adapt_failures('inactive', theta, sup, cfg, 1, LR, 'tf1_slices', 'dense_norm')
    assert len(failures) == 1 and 'gnorm' in failures[0]


@pytest.mark.parametrize('idx', SHAPES)
def test_a_stale_recurrent_weight_image_fails_the_query_pass_check(idx):
    """point 2 of the issue: the query pass runs with K_h of layer 0 still at theta while Kx, the biases, the embedding and the
    softmax layer are theta' (khf_dirty dropped from sgd_update).  inner_lr 0.1."""
    shape, cfg, sup, qry, theta = setup(idx)
    fast, failures = MR.adapt_failures(MR.shape_id(shape), theta, sup, cfg, shape[4], LR, 'tf1_slices')
    assert not failures
    E = cfg['embedding_size']
    stale = {k: v.copy() for k, v in fast.items()}
    stale['kernel_0'][E:] = theta['kernel_0'][E:]
    ref = MR.query_reference(fast, qry, cfg)
    loss, got = MR.pass_tensors32(stale, qry, cfg)
    bad = MR.query_failures(ref, got, M)
    rel = abs(loss - ref.loss) / abs(ref.loss)
    print('STALE|%s|loss off by %.1e relative (%s by the 1e-4 loss bound)|%s' % (
        MR.shape_id(shape), rel, 'caught' if rel > NLL_RTOL else 'NOT caught',
        ', '.join('%s %.0f x e32' % (k, v[1]) for k, v in sorted(bad.items()))))
    assert rel <= NLL_RTOL          # the loss alone would have let it through, on every shape: the argument for the query-pass check
    # the states of layer 0 are the first thing a stale K_h changes, and everything behind them follows
    for fam in ('hs_0', 'cs_0', 'dz_0', 'logits', 'kernel_0'):
        assert fam in bad and bad[fam][1] > 10 * M, (fam, bad.get(fam))
