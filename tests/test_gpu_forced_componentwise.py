"""-m gpu: every recurrence kernel family against the fp64 oracle ELEMENT BY ELEMENT, at the row counts where its geometry changes.

tests/test_gpu_componentwise.py holds what the default dispatch picks at the 14 shapes of backward_ref.CW_SHAPES to M * e32 in every
element; the other kernels of the recurrence -- chosen by padded hidden size, row count and the knobs fsmg_create reads -- were held
norm-wise only.  Here the same measure, the same reference class, the same device reader and the same M = 8 run on

  (a) the row edges of the default dispatch (no knob): every row-group and row-tile edge of the XCD-local kernels at hidden 512 /
      1024 / 256, what the row counts above them get, row-tile edges of the column-split chains, and k_lstm_fwd_patch;
  (b) one launch per time step (FSMG_PERSISTENT=0) at Hp 64 .. 1024 -- what every handle runs after a recovered time-out;
  (c) the column-split persistent kernels where the XCD-local ones are the default (FSMG_XCD=0, FSMG_XCD_PAIR=0 / 1) and the
      all-row-tiles forward kernel (FSMG_FWD_RT=1);
  (d) the other arithmetic of the XCD-local kernels (FSMG_XCD_BX3, FSMG_XCD_VARIANT);
  (e) the XCD-partitioned order against the same reference object as the serial order on the same shape;
  (f) the pass repeated on per-step launches behind a timed-out XCD-local pass, and the first XCD-local pass after the fallback
      period (the inbox-refill situation), both element by element.

One GEMM arithmetic (the default bf16-split one): the GEMMs are not the subject.  Every case asserts which family ran, from
fsmg_stats and the debug reads, against backward_ref.expected_dispatch -- the dispatch of forward() / backward() restated, with the
rules written there and checked on the CPU by tests/test_forced_componentwise_cpu.py.  A case whose family did not run fails,
whatever its numbers are.  Measured figures: tests/COMPONENTWISE.md, "Forced families and row edges".
"""
import numpy as np
import pytest

import backward_ref as R
from conftest import small_config
from gpu_utils import new_model
from test_gpu_componentwise import M, check_all, device_tensors, reference

pytestmark = pytest.mark.gpu

assert M == 8                 # the project's number: no case here gets another
SPIN_LIMIT = 1 << 18          # fsmg_model::chain_spin_limit's default (fsmg_model.h)


def assert_family(model, cfg, B, env, passes=1, persist_now=None, timeouts=0, base=(0, 0, 0)):
    """the counters of fsmg_stats after `passes` forward_backward calls beyond `base` = (xcd, persistent, step launches), and the
    debug reads, against the restated dispatch.  Rule (backward_ref.expected_dispatch): without the two-stream order a layer's chain
    is ONE launch per direction on the XCD-local or the column-split persistent kernels, max_len launches per direction on per-step
    ones -- so a pass counts 2 L launches in one of the first two counters, or 2 L T in the third, or L of one and L (T) of another
    where the two directions differ (FSMG_XCD_PAIR=1)."""
    want = R.expected_dispatch(cfg, B, env, persist_now=persist_now)
    st = model.stats()
    assert model.debug_dims()['Hp'] == want['Hp']
    got = (st['xcd_launches'] - base[0], st['persistent_launches'] - base[1], st['step_launches'] - base[2])
    assert got == tuple(passes * want[k] for k in ('xcd_launches', 'persistent_launches', 'step_launches')), (got, want)
    assert st['timeouts'] == timeouts
    assert bool(model.debug_read('xcd_bx3', 1)[0]) == want['xcd_bx3'], want
    assert model.debug_read('xcd_partitioned', 3)[2] == float(want['xov']), want        # [2]: whether the LAST train pass took the order
    assert int(model.debug_read('xov_dk_tail', 4)[1]) == passes * int(want['dk_tail']), want        # [1]: joint dW + dK clean-up launches so far
    return want, st


def run_case(case, monkeypatch, ref_key=None):
    env, over, N, K, Q, seed = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # before new_model: fsmg_create reads them
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    ref = reference(ref_key, model, sup, qry, cfg)
    model.debug_set('inplace_dlogits', 0)          # keep the logits beside dlogits (and dlogits materialised: no fused softmax)
    model.forward_backward(sup, qry)
    want, st = assert_family(model, cfg, B, env)
    check_all('forced-%s|bx3' % R.forced_id(case), ref, device_tensors(model, cfg, B))
    return model, cfg, B, want, st


@pytest.mark.parametrize('case', R.FORCED_ROW_EDGES, ids=R.forced_id)
def test_row_edges_of_the_default_dispatch(case, monkeypatch):
    model, cfg, B, want, st = run_case(case, monkeypatch)
    H, T = cfg['hidden_size'], cfg['max_len']
    bx3 = bool(model.debug_read('xcd_bx3', 1)[0])
    if H == 512:
        # xcd_row_groups: ceil(ceil(B / 8) / 4), 3 padded to 4 -> 1 / 2 / 4 / 4 row groups up to 32 / 64 / 96 / 128 rows; the bf16-split
        # kernels from three row groups on (lstm_xcd_bx3_pays)
        if B <= 128:
            assert bx3 == (B > 64) and st['xcd_launches'] == 2 and st['persistent_launches'] == st['step_launches'] == 0
        else:
            # 129 rows are 9 row tiles: k_lstm_fwd_chain<8> would need 128 x 9 = 1152 blocks (921 fit), k_lstm_fwd_chain_rt takes 2 .. 4
            # row tiles, k_lstm_bwd_rs<4> 32 x 9 = 288 blocks (230 fit) -- so NO persistent kernel takes them: one launch per step
            assert st['xcd_launches'] == 0 and st['persistent_launches'] == 0 and st['step_launches'] == 2 * T
    elif H == 1024:
        # one weight copy per XCD pair: ceil(ceil(B / 4) / 4) row groups, the bf16-split pair kernels from three (33 rows) on
        assert bx3 == (B >= 33)
        if B <= 64:
            assert st['xcd_launches'] == 2 and st['persistent_launches'] == st['step_launches'] == 0
        else:       # 65 rows: 5 row tiles, past k_lstm_fwd_chain_rt's 4 and k_lstm_bwd_rs<8>'s 230 blocks (64 x 5)
            assert st['xcd_launches'] == 0 and st['persistent_launches'] == 0 and st['step_launches'] == 2 * T
    elif H == 256:
        # sixteen slices, 1 / 2 row groups up to 64 / 128 rows; above: k_lstm_fwd_chain<4> (64 x 9 blocks) + k_lstm_bwd_rs<2> (16 x 9)
        assert not bx3
        assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == ((2, 0, 0) if B <= 128 else (0, 2, 0))
    elif H == 128:
        assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (0, 2, 0)        # k_lstm_fwd_chain<2> + k_lstm_bwd_rs<1>
    else:
        # Hp stays 32 (2 k-groups do not split over 4 waves: no persistent kernel), 5 row tiles: launch_lstm_fwd_step takes k_lstm_fwd_patch
        assert (H, B, want['fwd']) == (32, 70, 'patch')
        assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (0, 0, 2 * T)


@pytest.mark.parametrize('case', R.FORCED_PER_STEP, ids=R.forced_id)
def test_per_step_launches(case, monkeypatch):
    model, cfg, B, want, st = run_case(case, monkeypatch)
    # T launches per layer and direction, nothing else
    assert st['xcd_launches'] == st['persistent_launches'] == 0 and st['step_launches'] == 2 * cfg['max_len'] * cfg['n_layers']
    assert want['fwd'] == ('patch' if B >= 49 else 'step')          # k_lstm_fwd_patch<4, 2, 2> from 4 row tiles on


@pytest.mark.parametrize('case', R.FORCED_COLUMN_SPLIT, ids=R.forced_id)
def test_column_split_persistent_kernels(case, monkeypatch):
    model, cfg, B, want, st = run_case(case, monkeypatch)
    L = cfg['n_layers']
    if case[0].get('FSMG_XCD_PAIR') == '1':         # the pair kernel forward, k_lstm_bwd_rs<8> backward
        assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (L, L, 0)
    else:
        assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (0, 2 * L, 0)
    if 'FSMG_FWD_RT' in case[0] or (cfg['hidden_size'] == 1024 and B == 45 and case[0].get('FSMG_XCD_PAIR') == '0'):
        assert want['fwd'] == 'chain_rt'            # 3 (4) row tiles walked by one block per column tile


@pytest.mark.parametrize('case', R.FORCED_XCD_ARITH, ids=R.forced_id)
def test_other_arithmetic_of_the_xcd_local_kernels(case, monkeypatch):
    model, cfg, B, want, st = run_case(case, monkeypatch)
    assert bool(model.debug_read('xcd_bx3', 1)[0]) == (case[0]['FSMG_XCD_BX3'] == '1')
    assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (2 * cfg['n_layers'], 0, 0)


@pytest.mark.parametrize('case', R.FORCED_XOV, ids=R.forced_id)
def test_xcd_partitioned_order_and_the_serial_order_against_one_reference(case, monkeypatch):
    """"The same bits as the serial order" (tests/test_gpu_parity.py) is checked there with atol = 1e-5 * max, in which a stale row read by
    the gated projection or by dW's queue would be silent; here both orders are held to the fp64 reference -- one object per shape,
    asserted to be built from the same parameters -- in every element."""
    model, cfg, B, want, st = run_case(case, monkeypatch, ref_key='forced/' + R.shape_id(R.forced_shape(case)))
    assert (st['xcd_launches'], st['persistent_launches'], st['step_launches']) == (2, 0, 0)
    on = case[0]['FSMG_XCD_OVERLAP'] == '1'
    T = cfg['max_len']
    # choose_schedule: the chains packed 16 rows per XCD must leave three XCDs to the GEMMs (B <= 80); backward(): dW's K = T * B rows
    # split in pieces of 256 at least, two pieces at least; the joint clean-up launch where the merged dK takes the 256-tile kernel
    assert want['xov'] == (on and B <= 80) and want['xov_fwd'] == want['xov']
    assert want['xov_bwd'] == (want['xov'] and T * B >= 512)
    assert want['dk_tail'] == (want['xov_bwd'] and cfg['embedding_size'] == 250 and T * B >= 2048)
    assert st['xov_selfcheck_mismatches'] == 0
    if want['xov_bwd']:
        # the backward pair ran: every item of dW's queue -- 2 row tiles x column tiles x K pieces -- was claimed exactly once, by the
        # restricted launch beside the chain or by the clean-up launch behind it
        items = 2 * ((model.debug_dims()['V1p'] + 255) // 256) * want['dw_split']
        claims = model.debug_read('xov_bwd_queue', 4 + items)[4:]
        assert np.all(claims == 1.0), claims
    if want['dk_tail']:
        tail = model.debug_read('xov_dk_tail', 4)
        assert tail[1] >= 1 and tail[2] == 2 * ((model.debug_dims()['V1p'] + 255) // 256) * want['dw_split'] and tail[3] >= 48


def test_pass_repeated_after_a_time_out_and_the_first_pass_after_the_fallback_period(monkeypatch):
    """FSMG_CHAIN_SPIN_LIMIT=0 is the designed software time-out of tests/test_gpu_parity.py
    test_persistent_kernel_timeout_falls_back_and_repeats_the_step: the XCD-local kernels give up at their first wait, the update is
    skipped (code -9).  The pass repeated on per-step launches -- behind the abandoned partials of the XCD-local kernels -- and, after the
    fallback period, the first pass back on the XCD-local kernels -- on BPTT inboxes the aborted pass wrote into, the situation of
    test_inbox_refill_flag_survives_the_fallback_period -- are each held to the fp64 reference in every element.
    fallback_steps is 2, not 1: forward_backward_core counts the period down BEFORE it runs (`--fallback_left == 0` puts the persistent
    path back for the call that makes it), so with 1 the repeated pass itself would be back on the XCD-local kernels."""
    from fsmg.binding import FsmgError, RETRY_CODES
    env, over, N, K, Q, seed = R.FORCED_RECOVERY
    monkeypatch.setenv('FSMG_CHAIN_SPIN_LIMIT', '0')
    cfg = small_config(**over)
    T = cfg['max_len']
    sup, qry = R.episode(cfg, N, K, Q, seed)
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    ref = reference(None, model, sup, qry, cfg)
    model.debug_set('inplace_dlogits', 0)
    model.debug_set('fallback_steps', 2)
    model.forward_backward(sup, qry)
    with pytest.raises(FsmgError, match='persistent recurrent kernel timed out') as ei:
        model.apply_update(1.0)
    assert ei.value.code == -9 and ei.value.code in RETRY_CODES and model.step == 0
    st = model.stats()
    assert st['timeouts'] == 1 and st['xcd_launches'] == 2 and st['step_launches'] == 0 and not st['persistent_path']
    model.forward_backward(sup, qry)               # the repeat: 2 T per-step launches, no persistent one
    assert_family(model, cfg, B, env, persist_now=False, timeouts=1, base=(2, 0, 0))
    assert model.stats()['fallback_steps_left'] == 1
    check_all('forced-recovery-fallback|bx3', ref, device_tensors(model, cfg, B))
    # the period ends: the next pass -- a whole train step, on another episode -- puts the persistent path back
    model.debug_set('chain_spin_limit', SPIN_LIMIT)
    loss = model.train_step(*R.episode(cfg, N, K, Q, seed + 1))
    st = model.stats()
    assert np.isfinite(loss) and model.step == 1 and st['timeouts'] == 1 and st['persistent_path'] and st['fallback_steps_left'] == 0
    assert (st['xcd_launches'], st['step_launches']) == (4, 2 * T)
    ref2 = reference(None, model, sup, qry, cfg)   # at the parameters the update left
    assert any(not np.array_equal(ref2.params[k], ref.params[k]) for k in ref.params)
    model.forward_backward(sup, qry)
    assert_family(model, cfg, B, env, timeouts=1, base=(4, 0, 2 * T))
    check_all('forced-recovery-back|bx3', ref2, device_tensors(model, cfg, B))
