"""The deferred softmax half of clip + Adam and the trimmed hand-off refill, on the GPU.

Under the XCD-partitioned eager order (hidden 512, one layer) the fused train step launches [embedding .. LSTM layers] of the update
and leaves [softmax_w, softmax_b] NOT LAUNCHED; the next train pass puts it on the auxiliary stream behind the x-part GEMM, restricted
to the XCDs its forward chain leaves free, and every other entry point launches it in stream order first (settle_pending).  Same
operations on the same values: everything here is compared bit for bit against a handle with the in-line single launch.

The shape is the smallest at which the order is taken: it is asked for by name (the AUTO rule wants 32 time steps and 320 projection
tiles), 8 time steps, 20 rows = two XCDs of ten (12 rows = one XCD, 36 = three), one 256-row tile of the projection."""
import numpy as np
import pytest

from conftest import small_config
from gpu_utils import new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

CFG = dict(hidden_size=512, embedding_size=32, input_size=3000, max_len=8)
NKQ = (5, 2, 2)          # 20 rows


def _pair(defer_a=1, defer_b=0):
    cfg = small_config(**CFG)
    a = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
    b = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
    assert a.debug_read('xcd_partitioned', 1)[0] == 1.0 and b.debug_read('xcd_partitioned', 1)[0] == 1.0
    a.debug_set('upd_defer', defer_a)
    b.debug_set('upd_defer', defer_b)
    return cfg, a, b


def _episodes(cfg, n, nkq=NKQ, seed=61):
    return O.synthetic_episodes(n, nkq[0], nkq[1], nkq[2], cfg['max_len'], cfg['input_size'], seed=seed)


def _state(m):
    """[knob, the half when the call began (0 none, 1 in flight, 2 not launched), halves placed beside a chain, halves settled in line]"""
    return [int(v) for v in m.debug_read('upd_defer', 4)]


def _same_model(a, b):
    pa, pb = a.get_params(), b.get_params()
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)
        (ma, va), (mb, vb) = a.get_opt_state(k), b.get_opt_state(k)
        np.testing.assert_array_equal(ma, mb, err_msg='m ' + k)
        np.testing.assert_array_equal(va, vb, err_msg='v ' + k)


def test_three_steps_deferred_equal_three_steps_in_line_bit_for_bit():
    cfg, a, b = _pair()
    eps = _episodes(cfg, 3)
    la = [a.train_step(s_, q_) for s_, q_ in eps]
    lb = [b.train_step(s_, q_) for s_, q_ in eps]
    sa, sb = _state(a), _state(b)                                   # (first: any other read settles the waiting half)
    assert int(a.debug_read('xcd_partitioned', 3)[2]) == 1          # the order was taken
    assert sa[0] == 1 and sa[1] == 2 and sa[2] == 2                 # the last half waits, the two before it ran beside a forward chain
    assert sb == [0, 0, 0, 0]
    assert la == lb
    assert a.step == b.step == 3
    np.testing.assert_array_equal(a.read_losses(3), b.read_losses(3))
    _same_model(a, b)
    assert _state(a)[1] == 0 and _state(a)[3] == 1
    st = a.stats()
    assert st['timeouts'] == 0 and st['xov_selfcheck_mismatches'] == 0


def test_every_reader_settles_the_waiting_half():
    cfg, a, b = _pair()
    eps = _episodes(cfg, 12, seed=62)
    qry = eps[0][1]
    rows = eps[1][0].reshape(-1, cfg['max_len'])

    def both(f):
        ra, rb = f(a), f(b)
        return ra, rb

    def check_scores(m):
        return m.score(rows, rank=True, entropy=True)

    readers = [
        ('get_param', lambda m: m.get_param('softmax_w')),
        ('set_param', lambda m: m.set_param('softmax_b', np.full(cfg['input_size'] + 1, 0.01, np.float32))),
        ('get_opt_state', lambda m: np.stack(m.get_opt_state('softmax_w'))),
        ('eval', lambda m: m.eval_step(qry)),
        ('forward_backward', lambda m: (m.forward_backward(*eps[2]), m.apply_update(1.0))[1]),
        ('score', check_scores),
        ('generate', lambda m: m.generate(3, 6, temperature=0.9, seed=5)),
        ('maml_eval', lambda m: m.maml_eval(eps[3][0], eps[3][1], 1, 0.1)),          # save theta, adapt, restore theta
        ('stats', lambda m: m.stats()['steps_skipped_token_range']),
        ('step', lambda m: m.step),
    ]
    for i, (name, f) in enumerate(readers):
        s_, q_ = eps[4 + (i % 8)]
        assert a.train_step(s_, q_) == b.train_step(s_, q_), name
        assert _state(a)[1] == 2, name                                  # a half is waiting, not launched
        ra, rb = both(f)
        if isinstance(ra, dict):
            for k in ra:
                np.testing.assert_array_equal(ra[k], rb[k], err_msg='%s %s' % (name, k))
        elif ra is not None:
            np.testing.assert_array_equal(np.asarray(ra), np.asarray(rb), err_msg=name)
        assert _state(a)[1] == 0, name                                  # nothing pending behind the call
        _same_model(a, b)
    assert a.train_step(*eps[0]) == b.train_step(*eps[0])
    assert _state(a)[1] == 2
    wa = a.get_param('softmax_w')
    a.close()                                                           # ends the handle's life with a half settled a call before
    np.testing.assert_array_equal(wa, b.get_param('softmax_w'))
    c = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
    c.train_step(*eps[0])
    assert _state(c)[1] == 2
    c.close()                                                           # ... and with one still waiting


def test_a_skipped_step_leaves_the_softmax_half_alone():
    cfg, a, b = _pair()
    eps = _episodes(cfg, 3, seed=63)
    assert a.train_step(*eps[0]) == b.train_step(*eps[0])
    names = ('softmax_w', 'softmax_b')
    before = {k: (b.get_param(k),) + b.get_opt_state(k) for k in names}
    bad = eps[1][0].copy(); bad[0, 0, 0] = cfg['input_size'] + 5
    for m in (a, b):
        with pytest.raises(Exception, match='TOKEN_RANGE'):
            m.train_step(bad, eps[1][1])
    assert a.stats()['steps_skipped_token_range'] == 1 and a.step == b.step == 1
    for k in names:
        got = (a.get_param(k),) + a.get_opt_state(k)
        for x, y in zip(got, before[k]):
            np.testing.assert_array_equal(x, y, err_msg=k)
    assert a.train_step(*eps[2]) == b.train_step(*eps[2])
    assert a.step == b.step == 2
    _same_model(a, b)


def test_hand_off_refill_follows_the_xcds_in_use():
    """Fewer -> more -> fewer XCDs on one handle: every pass finds the slices it uses "not written" and equals a fresh handle's."""
    cfg = small_config(**CFG)
    shapes = [(3, 2, 2), (4, 5, 4), (3, 2, 2), (5, 2, 2)]           # 12, 36, 12, 20 rows: one, three, one, two XCDs
    m = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
    for i, nkq in enumerate(shapes):
        B = nkq[0] * (nkq[1] + nkq[2])
        (s_, q_), = _episodes(cfg, 1, nkq, seed=70 + i)
        m.forward_backward(s_, q_)                                  # (no update in between: every pass starts from the seed's parameters)
        assert int(m.debug_read('xcd_partitioned', 3)[2]) == 1
        f = new_model(cfg, max_sequences=45, schedule='xcd_partitioned')
        f.forward_backward(s_, q_)
        n = (cfg['max_len'] + 1) * B * 512
        np.testing.assert_array_equal(m.debug_read('h0', n), f.debug_read('h0', n), err_msg='pass %d' % i)
        np.testing.assert_array_equal(m.debug_read('ce', cfg['max_len'] * B), f.debug_read('ce', cfg['max_len'] * B), err_msg='pass %d' % i)
        for k in m.param_shapes:
            np.testing.assert_array_equal(m.get_grad(k), f.get_grad(k), err_msg='pass %d %s' % (i, k))
        f.close()
