"""-m gpu: the entry points and the failure paths of the MAML-style step (cfg-E, api_step.hip).

  D1  fsmg_maml_step_indexed / fsmg_maml_forward_backward_indexed (gather_episode, k_gather_rows: the route train.train takes for
      MAMLLSTM) give the bits of the token forms on the gathered rows;
  D2  a token outside [0, input_size) -- in the support set, in the query set, as an index past the table -- is TOKEN_RANGE, and
      "theta comes back whatever happened": parameters, Adam slots and step are what they were, the next good step is the one a handle
      takes that never saw the bad episode;
  D3  a timed-out chain (the handle's own knob chain_spin_limit 0: the persistent kernels give up at their first wait, the library
      repeats the call once on per-step launches) inside fsmg_maml_step and fsmg_maml_eval.
"""
import numpy as np
import pytest

import maml_ref as MR
from gpu_utils import new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-4
LR = MR.INNER_LR


def state(m):
    return m.get_params(), {k: m.get_opt_state(k) for k in m.param_shapes}, m.step


def assert_same_state(a, b, what=''):
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)), (what, 'parameter', k)
        for slot in (0, 1):
            assert np.array_equal(a[1][k][slot].view(np.uint32), b[1][k][slot].view(np.uint32)), (what, 'Adam slot %d' % slot, k)
    assert a[2] == b[2], (what, 'step', a[2], b[2])


def setup(idx):
    shape = MR.MAML_SHAPES[idx]
    over, N, K, Q, n, seed = shape
    cfg = MR.config_of(shape)
    return shape, cfg, MR.initial_theta(cfg), N * (K + Q)


def songs(cfg, n, seed):
    (sup, _), = O.synthetic_episodes(1, n, 1, 1, cfg['max_len'], cfg['input_size'], seed=seed, realistic=True)
    return sup.reshape(n, cfg['max_len'])


# ----------------------------------------------------------------------------- D1
@pytest.mark.parametrize('idx', [1, 3])
def test_indexed_forms_equal_the_token_forms_bit_for_bit(idx):
    shape, cfg, theta, B = setup(idx)
    over, N, K, Q, n, seed = shape
    table = songs(cfg, 40, seed=5)
    a, b = new_model(cfg, theta, max_sequences=B), new_model(cfg, theta, max_sequences=B)
    b.upload_table(0, table)
    rng = np.random.RandomState(7)
    for s in range(3):
        si, qi = rng.randint(0, 40, size=(N, K)), rng.randint(0, 40, size=(N, Q))
        si[0, 0] = 39                              # the last row of the table
        qi[N - 1, Q - 1] = si[N - 1, K - 1]        # a song twice, in both sets
        if K > 1:
            si[0, 1] = si[0, 0]                    # ... and twice in one set
        want = a.maml_step(table[si], table[qi], n, LR)
        got = b.maml_step_indexed(0, si, qi, n, LR, want_loss=(s != 1))
        assert got == (want if s != 1 else None)
        assert_same_state(state(a), state(b), 'step %d' % s)
    np.testing.assert_array_equal(b.read_losses(3), a.read_losses(3))
    assert a.step == 3

    def split_forms(N2):
        si, qi = rng.randint(0, 40, size=(N2, K)), rng.randint(0, 40, size=(N2, Q))
        si[0, 0], qi[0, 0] = 39, 39
        before = state(b)
        a.maml_forward_backward(table[si], table[qi], n, LR)
        b.maml_forward_backward_indexed(0, si, qi, n, LR)
        for k in a.param_shapes:
            ga, gb = a.get_grad(k), b.get_grad(k)
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)) and np.abs(ga).max() > 0, k
        assert_same_state(state(b), before, 'theta untouched')
        assert_same_state(state(a), before)
    split_forms(N)
    split_forms(N + 2)                             # more rows than the handle has seen: the gather buffers and the scratch grow
    assert a.maml_step(table[:N * K].reshape(N, K, -1), table[:N * Q].reshape(N, Q, -1), n, LR) == \
        b.maml_step_indexed(0, np.arange(N * K).reshape(N, K), np.arange(N * Q).reshape(N, Q), n, LR)
    assert_same_state(state(a), state(b), 'after the larger episode')
    assert a.stats()['timeouts'] == 0 and b.stats()['timeouts'] == 0
    from fsmg.binding import FsmgError
    with pytest.raises(FsmgError, match='STATE'):
        b.maml_step_indexed(1, np.zeros((N, K), np.int32), np.zeros((N, Q), np.int32), n, LR)        # no table under this id


# ----------------------------------------------------------------------------- D2
@pytest.mark.parametrize('where', ['support', 'query'])
@pytest.mark.parametrize('idx', [1, 3])
def test_bad_tokens_leave_everything_as_it_was(idx, where):
    from fsmg.binding import FsmgError
    shape, cfg, theta, B = setup(idx)
    over, N, K, Q, n, seed = shape
    sup, qry = MR.episode(cfg, shape)
    sup2, qry2 = MR.episode(cfg, (over, N, K, Q, n, seed + 1))
    table = songs(cfg, 40, seed=5)
    a, clean = new_model(cfg, theta, max_sequences=B), new_model(cfg, theta, max_sequences=B)
    a.upload_table(0, table)
    assert a.maml_step(sup, qry, n, LR) == clean.maml_step(sup, qry, n, LR)            # Adam slots that are not zero
    before = state(a)
    bad_sup, bad_qry = sup.copy(), qry.copy()
    (bad_sup if where == 'support' else bad_qry)[N - 1, 0, 2] = cfg['input_size']         # the start word is no data token
    si, qi = np.arange(N * K).reshape(N, K), np.arange(N * Q).reshape(N, Q)
    (si if where == 'support' else qi)[0, 0] = 40                                          # one past the table
    skipped = 0
    for name, call, counts in [('maml_step', lambda: a.maml_step(bad_sup, bad_qry, n, LR), 1),
                               ('maml_eval', lambda: a.maml_eval(bad_sup, bad_qry, n, LR), 0),       # (no train step: nothing to skip)
                               ('maml_step_indexed', lambda: a.maml_step_indexed(0, si, qi, n, LR), 1)]:
        with pytest.raises(FsmgError, match='TOKEN_RANGE'):
            call()
        skipped += counts
        assert_same_state(state(a), before, name)
        assert a.stats()['steps_skipped_token_range'] == skipped, name
    assert a.maml_eval(sup2, qry2, n, LR) == clean.maml_eval(sup2, qry2, n, LR)
    assert a.maml_step(sup2, qry2, n, LR) == clean.maml_step(sup2, qry2, n, LR)
    assert_same_state(state(a), state(clean), 'the next good step')
    assert a.step == 2 and a.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- D3
def test_timed_out_chain_inside_maml_step_and_maml_eval():
    shape, cfg, theta, B = setup(3)                # hidden 512: the fp32 XCD-local kernels, passes of 15 and 10 rows
    over, N, K, Q, n, seed = shape
    eps = [MR.episode(cfg, (over, N, K, Q, n, seed + i)) for i in range(4)]
    a, b = new_model(cfg, theta, max_sequences=B), new_model(cfg, theta, max_sequences=B)
    params, opt = MR.f64(theta), O.new_opt_state(MR.f64(theta))

    def step(ep):
        """the oracle's loss inside 1e-4, and the bits of handle b, which runs the same kernel families and never times out (the
        parameters are held to b's bits and not to the oracle: an Adam step is sign-like, so the biases, which start at zero, carry
        the relative error of their smallest gradients -- 7.6e-4 of max|bias_0| was measured here after the three steps)"""
        want = O.maml_step(params, opt, ep[0], ep[1], cfg, n, LR)
        got = a.maml_step(ep[0], ep[1], n, LR)
        assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
        assert got == b.maml_step(ep[0], ep[1], n, LR)
        assert_same_state(state(a), state(b))

    step(eps[0])
    st = a.stats()
    assert st['xcd_launches'] + st['persistent_launches'] > 0 and st['timeouts'] == 0 and st['persistent_path']
    a.debug_set('chain_spin_limit', 0)
    before = state(a)
    want = O.maml_eval(params, eps[1][0], eps[1][1], cfg, n, LR)
    got = a.maml_eval(eps[1][0], eps[1][1], n, LR)                # times out in the adaptation, repeated once on per-step launches
    assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
    st = a.stats()
    assert st['timeouts'] == 1 and not st['persistent_path']
    assert_same_state(state(a), before, 'maml_eval under the time-out')
    b.debug_set('persistent', 0)                                  # what the repeats run on
    assert got == b.maml_eval(eps[1][0], eps[1][1], n, LR)
    a.debug_set('persistent', 1)                                  # back on the persistent kernels, which give up again
    step(eps[2])
    st = a.stats()
    assert st['timeouts'] == 2 and not st['persistent_path'] and st['steps_skipped_timeout'] == 1
    assert a.step == before[2] + 1
    a.debug_set('chain_spin_limit', 1 << 18)
    a.debug_set('persistent', 1)
    b.debug_set('persistent', 1)
    x0 = st['xcd_launches'] + st['persistent_launches']
    step(eps[3])                                                  # (on BPTT inboxes that still hold the aborted passes' partials)
    st = a.stats()
    assert st['timeouts'] == 2 and st['persistent_path'] and st['xcd_launches'] + st['persistent_launches'] > x0
    assert a.step == before[2] + 2 and b.stats()['timeouts'] == 0
