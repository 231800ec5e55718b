"""The backward pair's joint clean-up launch, on the GPU.

Under the XCD-partitioned order at hidden 512, one layer, the merged dK (dKx + dKh + db) no longer has a launch of its own: its items
are the tail of the work list that dW's clean-up launch drains behind the BPTT chain (k_gemm_bx3h_pair).  Same K split, same slabs,
same slab sums in the same order, and each item runs the statements of the kernel its GEMM takes alone -- so everything here is
compared bit for bit against a handle with fsmg_debug_set("xov_dk_tail", 0), which issues the two launches.

Shapes: hidden 512, one layer, E = 250 (Ep = 256), V1 = 1801 (V1p = 1804: 8 column tiles, the last a sliver of 12), and
  B = 45, T = 46: 2070 rows -- the fewest time steps at which dW (K >= 2048) and with it the fused softmax and the merged dK take the
                  256-tile kernel; three XCDs of chain, five of GEMMs
  B = 20, T = 103: 2060 rows; two XCDs of chain, six of GEMMs
dW (512, 1804, K) in four K slabs = 64 items, dK (768, 2048, K) = 24 tiles x gemm()'s K split.  The order is asked for by name (AUTO
wants 320 projection tiles).

dW does not go through the two-part-A instantiation at all (the joint kernel branches per item to the statements of <XC, XC, BUFM = 3>
for dW and of <..., AG> for dK), so there is no AG-against-plain comparison of dW to make: the on / off comparison below covers both.
"""
import numpy as np
import pytest

import backward_ref as R
from conftest import small_config
from gpu_utils import new_model
from test_gpu_componentwise import check_all, device_tensors, reference

pytestmark = pytest.mark.gpu

BASE = dict(input_size=1800, embedding_size=250, hidden_size=512, n_layers=1)
SHAPES = {'b45_t46': (dict(BASE, max_len=46), 5, 5, 4), 'b20_t103': (dict(BASE, max_len=103), 5, 2, 2)}
IDS = sorted(SHAPES)


def _model(cfg, knob):
    m = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
    assert m.debug_read('xcd_partitioned', 1)[0] == 1.0
    m.debug_set('xov_dk_tail', knob)
    return m


def _tail(m):
    """[knob, joint launches enqueued, dW items, dK items of the last pass that took the tail]"""
    return [int(v) for v in m.debug_read('xov_dk_tail', 4)]


def _kinds(m):
    return [int(v) for v in m.debug_read('gemm_kinds', 4)]


def _took_the_order(m):
    assert int(m.debug_read('xcd_partitioned', 3)[2]) == 1
    assert list(m.debug_read('fused_softmax', 2)) == [1.0, 1.0]
    st = m.stats()
    assert st['timeouts'] == 0 and st['xov_selfcheck_mismatches'] == 0


def _same(a, b, what, grads):
    if grads:
        for k in a.param_shapes:
            np.testing.assert_array_equal(a.get_grad(k), b.get_grad(k), err_msg='%s: grad %s' % (what, k))
        np.testing.assert_array_equal(a.debug_read('tail', 2), b.debug_read('tail', 2), err_msg=what + ': tail')
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg='%s: %s' % (what, k))


@pytest.mark.parametrize('name', IDS)
def test_joint_launch_equals_the_two_launches_bit_for_bit(name):
    over, N, K, Q = SHAPES[name]
    cfg = small_config(**over)
    eps = [R.episode(cfg, N, K, Q, seed) for seed in (3, 4, 5, 6)]
    a, b = _model(cfg, 1), _model(cfg, 0)
    k0a, k0b = _kinds(a), _kinds(b)
    # step 1 in two calls, so that the gradients can be read
    a.forward_backward(*eps[0])
    b.forward_backward(*eps[0])
    ta, tb = _tail(a), _tail(b)
    d = a.debug_dims()
    assert (d['Ep'], d['Hp'], d['V1p']) == (256, 512, 1804)
    assert ta[:2] == [1, 1] and ta[2] == 2 * 8 * 4 and ta[3] >= 2 * 24 and ta[3] % 24 == 0, ta       # the joint launch ran: dW's 64 items, dK's 24 tiles x its K split
    assert tb == [0, 0, 0, 0], tb
    ka, kb = [x - y for x, y in zip(_kinds(a), k0a)], [x - y for x, y in zip(_kinds(b), k0b)]
    assert ka[:3] == kb[:3] and ka[3] == kb[3] - 1, (ka, kb)                                           # one launch of the 256-tile family fewer
    _took_the_order(a)
    _took_the_order(b)
    _same(a, b, 'pass 1', grads=True)
    assert a.apply_update(1.0) == b.apply_update(1.0)
    _same(a, b, 'step 1', grads=False)
    # steps 2 and 3 as fused train steps
    for s_, q_ in eps[1:3]:
        assert a.train_step(s_, q_) == b.train_step(s_, q_)
    assert a.step == b.step == 3
    _same(a, b, 'step 3', grads=False)
    # ... and the gradients of a fourth pass from there
    a.forward_backward(*eps[3])
    b.forward_backward(*eps[3])
    _same(a, b, 'pass 4', grads=True)
    assert _tail(a)[1] == 4 and _tail(b)[1] == 0
    _took_the_order(a)
    _took_the_order(b)


@pytest.mark.parametrize('name', IDS)
def test_gradients_with_the_joint_launch_against_the_fp64_oracle(name, monkeypatch):
    """every gradient tensor element by element, the bounds of tests/test_gpu_componentwise.py (M x e32 of the fp32 restatement)"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    over, N, K, Q = SHAPES[name]
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, 3)
    m = _model(cfg, 1)
    ref = reference(None, m, sup, qry, cfg)
    m.forward_backward(sup, qry)
    assert _tail(m)[:2] == [1, 1]
    _took_the_order(m)
    check_all('dk_tail-%s|bx3' % name, ref, device_tensors(m, cfg, N * (K + Q), with_intermediates=False))


@pytest.mark.parametrize('name', IDS)
def test_restricted_launch_leaves_every_dk_claim_word_zero(name):
    """knob value 2 leaves the clean-up launch out (the gradients of that pass are not computed): what is marked in the queue words
    then is what the restricted launch beside the chain took -- it is dW's launch alone, its work limit dW's item count"""
    over, N, K, Q = SHAPES[name]
    cfg = small_config(**over)
    m = _model(cfg, 2)
    m.forward_backward(*R.episode(cfg, N, K, Q, 3))
    knob, launches, n0, n1 = _tail(m)
    assert (knob, launches, n0) == (2, 0, 64) and n1 >= 48
    w = m.debug_read('xov_bwd_queue', 4 + n0 + n1).astype(np.int64)
    claims = w[4:]
    print('%s: restricted draws %d, claimed %d of %d dW items' % (name, w[0], claims[:n0].sum(), n0))
    assert w[1] == 0                                             # nobody drew from the clean-up counter
    assert set(claims[:n0].tolist()) <= {0, 1} and claims[:n0].sum() == min(w[0], n0)
    assert not claims[n0:].any()
    m.close()
