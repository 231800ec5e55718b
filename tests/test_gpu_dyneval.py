"""-m gpu: dynamic evaluation (include/fsmg.h "dynamic evaluation") against tests/dyneval_ref.py.

Shapes: the model dims of the first five maml_ref.MAML_SHAPES plus the hidden-1024 one (T of 4 to 7), with streams whose blocks take
every recurrence family: per-step launches, column-split, slice, the fp32 XCD-local kernels (15 rows at hidden 512), the bf16-split
ones (a block of 80 rows at hidden 512) and the pair kernels (a block of 35 rows at hidden 1024).  first_reported falls inside a
block of the rows_per_step grid, one row of a block ends before a window's lo (all-zero weights in a live pass), one block's later
windows are all empty (skipped), and T = 7 with S = 3 has the partial last window [6, 7).

Laws, bitwise: L1 lr = decay = 0 leaves theta_l = theta; L2 seg_len = T on one block is the one-pass masked call's pass; L3 tokens
behind a song's end never matter; L4 the window's weights, n_valid and the zero rows of dlogits; L5 theta, the Adam slots and the step
after any call, a refused one included; L6 graph replay gives the eager bits across changing windows; L7 eval_step is N score calls;
L8 generate is adapt, set_params, generate; L9 adapt_reported = 0 with first_reported = 0 scores at theta.

The update's arithmetic from the device's own values (dyneval_ref.update_check: the bound is derived there from the kernel's
operation count), both rules, the clip active and inactive, decay in {0, 0.02, 1}, the 1 / decay cap active on a planted element.

Against fp64: out_nll within NLL_RTOL = 1e-4; per tensor rel_max(theta_l) under max(REL_MAX = 5e-4, 8 x e32), e32 the error of the same
restatement in fp32 numpy on the same inputs (the cache tests' convention: several RMS updates compound); the reported log-probs
under max(NLL_RTOL x |fp64|, 8 x e32) element by element.  Every case prints e32 and the device's error (tests/COMPONENTWISE_DYNEVAL.md).
"""
import os

import numpy as np
import pytest
import yaml

import dyneval_ref as D
import maml_ref as MR
import masked_ref as KR
from gpu_utils import new_model, rel_max
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-4             # tests/test_gpu_parity.py
REL_MAX = 5e-4              # tests/test_gpu_maml_componentwise.py
NONE = np.zeros(1, np.int32)[:0]
SGD_LR, RMS_LR = 0.1, 0.002          # RMS divides by sqrt(ms / count) ~ 1e-2: the same order of step
# rows of the stream per shape: (R, first_reported) -- first_reported leaves a block of 80 rows at hidden 512 and of 35 at hidden 1024
ROWS = {0: (5, 1), 1: (5, 3), 2: (6, 1), 3: (15, 7), 4: (85, 80), 5: (40, 35)}
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, what):
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def case(idx, R=None):
    """(cfg, theta fp32, tokens [R, T], lengths [R]): the first rows (2, T) -- row 0 ends before the window [3, 6) -- and, from row 2 on,
    seeded lengths that hold a T"""
    key = ('case', idx, R)
    if key not in _cache:
        shape = MR.MAML_SHAPES[idx]
        cfg = MR.config_of(shape)
        T = cfg['max_len']
        R_ = R or ROWS[idx][0]
        rng = np.random.RandomState(500 + idx)
        tokens = rng.randint(0, cfg['input_size'], size=(R_, T)).astype(np.int32)
        lengths = rng.randint(1, T + 1, size=R_).astype(np.int32)
        lengths[:2] = (2, T)
        lengths[-1] = T
        _cache[key] = (cfg, MR.initial_theta(cfg), tokens, lengths)
    return _cache[key]


def stats_for(theta, count=4, big=False):
    """seeded positive ms_sum per parameter, fp32; big: one large element (the 1 / decay cap is active there)"""
    rng = np.random.RandomState(7)
    ms = {k: (rng.uniform(0.2, 2.0, size=np.shape(v)) * count * 1e-4).astype(np.float32) for k, v in sorted(theta.items())}
    if big:
        ms['softmax_w'].reshape(-1)[3] = 1e4
    return dict(count=count, ms_sum=ms)


def handle(cfg, theta, R, stats=None, mode='tf1_slices', **kw):
    m = new_model(cfg, theta, max_sequences=R, clip_norm_mode=mode, **kw)
    m.debug_set('keep_adapted', 1)
    if stats is not None:
        for k, v in stats['ms_sum'].items():
            m.dyneval_stats_set(k, v)
        m.dyneval_stats_set_count(stats['count'])
    return m


def adapted(m):
    return {k: m.get_adapted(k) for k in m.param_shapes}


def state(m):
    out = {'p:' + k: m.get_param(k) for k in m.param_shapes}
    for k in m.param_shapes:
        out['m:' + k], out['v:' + k] = m.get_opt_state(k)
    out['step'] = np.int64(m.step)
    return out


def score(m, dcfg, tokens, lengths, first):
    before = state(m)
    out = m.dyneval_score(dcfg, tokens, lengths, first_reported=first)
    same_bits(state(m), before, 'theta, the Adam slots and the step after the call')          # L5
    with pytest.raises(Exception, match='STATE'):
        m.apply_update(1.0)                                                                    # no gradient is pending
    row, nll = D.host_nll(out['logprob'], lengths, first)
    assert np.array_equal(bits(out['row_nll']), bits(row)) and (np.float32(out['nll']) == nll or (np.isnan(nll) and np.isnan(out['nll'])))
    assert np.all(out['logprob'][:first] == 0)
    T = tokens.shape[1]
    ln = np.full(len(tokens), T) if lengths is None else np.asarray(lengths)
    assert np.all(out['logprob'][np.arange(T)[None, :] >= ln[:, None]] == 0)
    out['theta_l'] = adapted(m)
    return out


# ----------------------------------------------------------------------------- L1, L9
@pytest.mark.parametrize('idx,rule', [(0, 'sgd'), (2, 'rms'), (3, 'rms')], ids=str)
def test_zero_lr_and_decay_leave_theta_and_unadapted_scores(idx, rule):
    cfg, theta, tokens, lengths = case(idx)
    R, first = ROWS[idx]
    m = handle(cfg, theta, R, stats_for(theta))
    still = score(m, dict(rule=rule, seg_len=3, rows_per_step=2, lr=0.0, decay=0.0), tokens, lengths, first)
    same_bits(still['theta_l'], theta, 'theta_l with lr = decay = 0')
    # L9: nothing adapts -> the log-probs of an unadapted pass (one window per block), and they are the zero-rate run's on the reported rows
    plain = score(m, dict(rule=rule, seg_len=3, rows_per_step=2, lr=SGD_LR, decay=0.02, adapt_reported=False), tokens, lengths, 0)
    same_bits(plain['theta_l'], theta, 'theta_l with adapt_reported = 0 and first_reported = 0')
    ce = np.zeros(tokens.shape, np.float32)
    for r0, r1, _ in D.blocks_of(R, 0, 2):
        m.forward_backward_masked(tokens[None, r0:r1], tokens[None, r0:r1], lengths[r0:r1], NONE, shape=(1, r1 - r0, 0))
        ce[r0:r1] = m.debug_read('ce', (r1 - r0) * tokens.shape[1]).reshape(tokens.shape[1], r1 - r0).T
    mask = np.arange(tokens.shape[1])[None, :] < lengths[:, None]
    assert np.array_equal(bits(plain['logprob'][mask]), bits(-ce[mask]))
    assert m.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- L2
@pytest.mark.parametrize('idx', [1, 3, 5], ids=str)
def test_one_window_over_one_block_is_the_masked_pass(idx):
    cfg, theta, tokens, lengths = case(idx)
    R, T = ROWS[idx][0], cfg['max_len']
    a, b = handle(cfg, theta, R), handle(cfg, theta, R)
    out = score(a, dict(rule='sgd', seg_len=T, rows_per_step=R, lr=SGD_LR, decay=0.02, clip_norm=MR.MAX_GRAD_NORM), tokens, lengths, 0)
    b.forward_backward_masked(tokens[None], tokens[None], lengths, NONE, shape=(1, R, 0))
    same_bits({k: a.get_grad(k) for k in a.param_shapes}, {k: b.get_grad(k) for k in b.param_shapes}, 'the gradient buffer')
    ce_a, ce_b = a.debug_read('ce', R * T), b.debug_read('ce', R * T)
    assert np.array_equal(bits(ce_a), bits(ce_b))
    assert np.array_equal(bits(a.debug_read('tail', 16)[:2]), bits(b.debug_read('tail', 16)[:2]))
    mask = np.arange(T)[None, :] < lengths[:, None]
    assert np.array_equal(bits(out['logprob'][mask]), bits(-ce_b.reshape(T, R).T[mask]))
    assert max(rel_max(out['theta_l'][k], theta[k]) for k in theta if not k.startswith('bias_')) > 1e-4      # it did adapt


# ----------------------------------------------------------------------------- L3
@pytest.mark.parametrize('idx,rule', [(0, 'sgd'), (3, 'rms')], ids=str)
def test_tokens_behind_a_songs_end_never_matter(idx, rule):
    cfg, theta, tokens, lengths = case(idx)
    R, first = ROWS[idx]
    other = KR.scramble_padding(tokens, lengths, cfg['input_size'], np.random.RandomState(91))
    assert not np.array_equal(other, tokens)
    dcfg = dict(rule=rule, seg_len=3, rows_per_step=2, lr=SGD_LR if rule == 'sgd' else RMS_LR, decay=0.02, clip_norm=MR.MAX_GRAD_NORM)
    outs = []
    for tk in (tokens, other):
        m = handle(cfg, theta, R, stats_for(theta))
        outs.append(score(m, dcfg, tk, lengths, first))
        same_bits(m.get_params(), theta, 'theta afterwards')
    assert np.array_equal(bits(outs[0]['logprob']), bits(outs[1]['logprob']))
    same_bits(outs[0]['theta_l'], outs[1]['theta_l'], 'theta_l')


# ----------------------------------------------------------------------------- L4
@pytest.mark.parametrize('idx,seg,want_window', [(0, 3, (6, 7)), (2, 3, (6, 7)), (1, 3, (3, 6)), (0, 1, (6, 7))], ids=str)
def test_window_weights_n_valid_and_zero_rows_of_dlogits(idx, seg, want_window):
    cfg, theta, tokens, lengths = case(idx)
    T, B = cfg['max_len'], 3
    m = handle(cfg, theta, B)
    m.debug_set('inplace_dlogits', 0)
    V1p = m.debug_dims()['V1p']
    ln = np.array([2, T, T - 1], np.int32)               # row 0 ends before every window but the first: all-zero weights in live passes
    score(m, dict(rule='sgd', seg_len=seg, rows_per_step=B, lr=SGD_LR), tokens[:B], ln, 0)
    lo, hi = want_window                                 # the last live window of the one block: what the buffers hold now
    assert D.windows_of(T, seg)[-1] == (lo, hi) or ln.max() <= D.windows_of(T, seg)[-1][0]
    e = np.minimum(ln, hi)
    inside = (np.arange(T)[:, None] >= lo) & (np.arange(T)[:, None] < e[None, :])          # [t, b]: device row order
    n_valid = int(inside.sum())
    assert n_valid > 0 and not inside[:, 0].any()
    w = m.debug_read('row_weight', T * B).reshape(T, B)
    assert m.debug_read('n_valid', 1)[0] == n_valid
    assert np.all(w[~inside] == 0) and np.array_equal(bits(w[inside]), bits(np.full(n_valid, np.float32(1.0 / (n_valid + 1e-12)))))
    assert m.debug_read('fused_softmax', 2)[1] == 0                                       # dlogits was materialised
    d = m.debug_read('dlogits', B * T * V1p).reshape(T, B, V1p)
    assert np.all(d[~inside] == 0) and np.all(np.abs(d[inside]).max(axis=-1) > 0)


# ----------------------------------------------------------------------------- L5: refusals
def test_refused_calls_touch_nothing():
    cfg, theta, tokens, lengths = case(0)
    R, T = ROWS[0][0], cfg['max_len']
    m = handle(cfg, theta, R)
    m.train_step(tokens[None, :3], tokens[None, 3:])             # Adam slots and a step that are not zero
    before = state(m)
    good = dict(rule='sgd', seg_len=3, rows_per_step=2, lr=0.1, decay=0.02)
    bad_lengths = lengths.copy()
    bad_lengths[2] = T + 1
    bad_tokens = tokens.copy()
    bad_tokens[1, 1] = cfg['input_size']
    cases = [(dict(good, seg_len=0), tokens, lengths, 1, 'INVALID'), (dict(good, seg_len=T + 1), tokens, lengths, 1, 'INVALID'),
             (dict(good, rows_per_step=0), tokens, lengths, 1, 'INVALID'), (dict(good, lr=-1.0), tokens, lengths, 1, 'INVALID'),
             (dict(good, decay=1.5), tokens, lengths, 1, 'INVALID'), (dict(good, rule='rms', eps=0.0), tokens, lengths, 1, 'INVALID'),
             (good, tokens, bad_lengths, 1, 'INVALID'), (good, tokens, lengths, R + 1, 'INVALID'), (good, tokens, lengths, -1, 'INVALID'),
             (good, bad_tokens, lengths, 1, 'TOKEN_RANGE'), (dict(good, rule='rms'), tokens, lengths, 1, 'STATE')]          # RMS with count == 0
    for dcfg, tk, ln, first, what in cases:
        with pytest.raises(Exception, match=what):
            m.dyneval_score(dcfg, tk, ln, first_reported=first)
        same_bits(state(m), before, 'after a refused call')
    with pytest.raises(Exception, match='INVALID'):
        m.dyneval_eval_step(dict(good, seg_len=T + 1), tokens[None, :3], tokens[None, 3:])
    with pytest.raises(Exception, match='STATE'):
        m.dyneval_stats_accumulate()                              # no gradient is pending
    same_bits(state(m), before, 'after the refused calls')
    assert m.dyneval_stats_info() == (0, 0.0)


# ----------------------------------------------------------------------------- L6
def test_graph_replay_gives_the_eager_bits_across_changing_windows(monkeypatch):
    cfg, theta, tokens, lengths = case(1)
    R, first = ROWS[1]
    dcfg = dict(rule='rms', seg_len=2, rows_per_step=2, lr=RMS_LR, decay=0.02, clip_norm=MR.MAX_GRAD_NORM)
    eager = score(handle(cfg, theta, R, stats_for(theta)), dcfg, tokens, lengths, first)
    monkeypatch.setenv('FSMG_EAGER', '0')
    m = handle(cfg, theta, R, stats_for(theta), use_graph=True)
    for rep in range(2):                                          # the first call captures the window passes, the second replays them
        got = score(m, dcfg, tokens, lengths, first)
        assert np.array_equal(bits(got['logprob']), bits(eager['logprob'])), rep
        same_bits(got['theta_l'], eager['theta_l'], 'theta_l, call %d' % rep)
    assert m.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- L7
@pytest.mark.parametrize('idx', [1, 3], ids=str)
def test_eval_step_is_one_score_call_per_artist(idx):
    shape = MR.MAML_SHAPES[idx]
    cfg = MR.config_of(shape)
    over, N, K, Q = shape[:4]
    T = cfg['max_len']
    sup, qry = (a.astype(np.int32) for a in MR.episode(cfg, shape))
    rng = np.random.RandomState(3)
    sl, ql = KR.lengths_for(rng, (N, K), T), KR.lengths_for(rng, (N, Q), T)
    theta = MR.initial_theta(cfg)
    dcfg = dict(rule='sgd', seg_len=3, rows_per_step=2, lr=SGD_LR, decay=0.02, clip_norm=MR.MAX_GRAD_NORM)
    m = handle(cfg, theta, N * (K + Q))
    got = m.dyneval_eval_step(dcfg, sup, qry, sl, ql)
    total, count = 0.0, 0
    for n in range(N):
        out = score(m, dcfg, np.concatenate([sup[n], qry[n]]), np.concatenate([sl[n], ql[n]]), K)
        for r in range(K, K + Q):
            for t in range(int(ql[n, r - K])):
                total += float(out['logprob'][r, t])
        count += int(ql[n].sum())
    assert np.float32(got) == np.float32(-total / count)
    full = m.dyneval_eval_step(dcfg, sup, qry)                    # NULL lengths: every song has T positions
    assert np.isfinite(full) and full != got
    same_bits(m.get_params(), theta, 'theta afterwards')


# ----------------------------------------------------------------------------- L8
@pytest.mark.parametrize('idx', [0, 3], ids=str)
def test_generate_is_adapt_then_generate_at_theta_l(idx):
    cfg, theta, tokens, lengths = case(idx)
    R = ROWS[idx][0]
    dcfg = dict(rule='sgd', seg_len=3, rows_per_step=2, lr=SGD_LR, decay=0.02, clip_norm=MR.MAX_GRAD_NORM)
    m = handle(cfg, theta, R)
    before = state(m)
    kw = dict(n_seq=3, temperature=0.9, top_k=5, seed=11, logprobs=True, top_p=0.9)
    toks, lp = m.dyneval_generate(dcfg, tokens, 4, support_len=lengths, **kw)
    theta_l = adapted(m)
    same_bits(state(m), before, 'after dyneval_generate')
    ref = score(m, dcfg, tokens, lengths, R)                      # nothing reported: the same adaptation
    same_bits(ref['theta_l'], theta_l, 'theta_l of generate and of score')
    assert np.isnan(ref['nll'])
    b = new_model(cfg, theta_l, max_sequences=R)
    toks2, lp2 = b.generate(num=4, **kw)
    assert np.array_equal(toks, toks2) and np.array_equal(bits(lp), bits(lp2))
    assert max(rel_max(theta_l[k], theta[k]) for k in theta if not k.startswith('bias_')) > 1e-4


# ----------------------------------------------------------------------------- the update's arithmetic, from the device's own values
# The clip must be ACTIVE where a case says so.  From the fp64 restatement at initial_theta(), the two windows' gradient norms of the
# blocks this test runs: 0.34 / 0.73 (shape 0), 0.35 / 0.44, 0.38 / 0.52, 0.38 / 0.58 (shape 3) over 4 rows -- above maml_ref's 0.3 --
# and 0.097 / 0.129 over the 80 rows at hidden 512, 0.133 / 0.192 over the 35 at hidden 1024: a mean over more positions is smaller, so
# the big blocks get a clip of their own below both.
BIG_BLOCK_CLIP = 0.05
UPDATE_CASES = [(0, 'sgd', 0.0, MR.MAX_GRAD_NORM, 'tf1_slices'), (0, 'rms', 0.02, MR.MAX_GRAD_NORM_INACTIVE, 'tf1_slices'),
                (1, 'sgd', 1.0, MR.MAX_GRAD_NORM_INACTIVE, 'dense'), (2, 'rms', 1.0, MR.MAX_GRAD_NORM, 'dense'),
                (3, 'rms', 0.0, MR.MAX_GRAD_NORM, 'tf1_slices'), (4, 'sgd', 0.02, BIG_BLOCK_CLIP, 'tf1_slices'),
                (5, 'rms', 0.02, BIG_BLOCK_CLIP, 'tf1_slices'), (1, 'sgd', 0.02, 0.0, 'tf1_slices')]


@pytest.mark.parametrize('idx,rule,decay,clip,mode', UPDATE_CASES, ids=str)
def test_update_arithmetic_from_the_devices_own_values(idx, rule, decay, clip, mode):
    """Two updates in one call (one block, windows [0, 2) and [2, T)): the second starts from a theta_l that differs from theta_g, so the
    pull-back term is live.  Its inputs are the device's own: theta_l before it = the kept theta_l of the same call cut after the first
    window (lengths 2: the second window is empty and skipped), its gradient = what the call left in the gradient buffer."""
    cfg, theta, tokens, lengths = case(idx)
    R, first = ROWS[idx]
    B = first if first >= 35 else min(R, 4)                      # the big blocks at hidden 512 / 1024, a few rows elsewhere
    T = cfg['max_len']
    stats = stats_for(theta, big=True)
    tk, ln = tokens[:B], np.maximum(lengths[:B], 3)              # every row reaches into the second window
    dcfg = dict(rule=rule, seg_len=2, rows_per_step=B, lr=SGD_LR if rule == 'sgd' else RMS_LR, decay=decay, eps=1e-3, clip_norm=clip)
    ref_cfg = D.dyn_config(rule=D.RMS if rule == 'rms' else D.SGD, seg_len=2, rows_per_step=B, lr=dcfg['lr'], decay=decay, eps=1e-3, clip_norm=clip)
    m = handle(cfg, theta, R, stats, mode)
    count, mean_rms = m.dyneval_stats_info()
    assert count == stats['count']
    # after the first window only: lengths clipped to 2 make every later window empty
    first_only = score(m, dcfg, tk, np.minimum(ln, 2), B)['theta_l']
    g1 = {k: m.get_grad(k) for k in m.param_shapes}
    failures = D.update_check('%d|%s|w0' % (idx, rule), theta, theta, g1, m.debug_read('tail', 16), mode, ref_cfg, stats, mean_rms,
                              first_only, m.debug_read('gnorm', 1)[0])
    # ... and the first two windows: lengths clipped to 4 (T >= 4 everywhere)
    both = score(m, dcfg, tk, np.minimum(ln, 4), B)['theta_l']
    g2 = {k: m.get_grad(k) for k in m.param_shapes}
    gnorm2 = m.debug_read('gnorm', 1)[0]
    failures += D.update_check('%d|%s|w1' % (idx, rule), first_only, theta, g2, m.debug_read('tail', 16), mode, ref_cfg, stats, mean_rms,
                               both, gnorm2)
    assert not failures, '; '.join(failures)
    if clip > 0:                                                  # active / inactive as the case says
        assert (gnorm2 > clip) == (clip in (MR.MAX_GRAD_NORM, BIG_BLOCK_CLIP)), (gnorm2, clip)
    if rule == 'rms' and decay > 0:                               # the cap is active on the planted element, and only there
        r = np.sqrt(stats['ms_sum']['softmax_w'].astype(np.float64) / count) / mean_rms
        assert (r > 1.0 / decay).sum() == (1 if decay < 1 else (r > 1).sum()) and r.reshape(-1)[3] > 1.0 / decay
    assert max(rel_max(both[k], first_only[k]) for k in theta if not k.startswith('bias_')) > 1e-5
    assert m.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- the statistics
@pytest.mark.parametrize('idx', [0, 2], ids=str)
def test_statistics_accumulate_in_fp32_and_mean_rms(idx):
    cfg, theta, tokens, lengths = case(idx)
    R = ROWS[idx][0]
    m = handle(cfg, theta, R)
    want = {k: np.zeros(np.shape(v), np.float32) for k, v in theta.items()}
    for i in range(3):
        if i == 1:
            m.forward_backward_masked(tokens[None, :3], tokens[None, 3:], lengths[:3], lengths[3:])
        else:
            m.forward_backward(tokens[None, i:i + 2], tokens[None, i + 2:])
        m.dyneval_stats_accumulate()
        for k in want:
            g = m.get_grad(k)
            want[k] = want[k] + g * g                             # fp32, two roundings, in the device's order
    got = {k: m.dyneval_stats_get(k) for k in want}
    same_bits(got, want, 'ms_sum after three passes')
    count, mean_rms = m.dyneval_stats_info()
    ref = D.mean_rms_of(dict(count=3, ms_sum=want))
    ulp = np.spacing(np.float32(ref))
    print('MEANRMS|%d|%.9g|%.9g|%.2f ulp' % (idx, mean_rms, ref, abs(mean_rms - ref) / ulp))
    assert count == 3 and abs(mean_rms - ref) <= 2 * ulp
    # set and get round-trip (the input has no pad elements: the reference layout), and the mean does not move
    b = handle(cfg, theta, R)
    for k, v in got.items():
        b.dyneval_stats_set(k, v)
    b.dyneval_stats_set_count(3)
    same_bits({k: b.dyneval_stats_get(k) for k in want}, got, 'set / get')
    assert np.float32(b.dyneval_stats_info()[1]) == np.float32(mean_rms)
    with pytest.raises(Exception, match='INVALID'):
        b.dyneval_stats_set('softmax_b', -np.ones(cfg['input_size'] + 1, np.float32))
    with pytest.raises(Exception, match='SIZE'):
        b.dyneval_stats_set('softmax_b', np.ones(3, np.float32))
    m.dyneval_stats_reset()
    assert m.dyneval_stats_info() == (0, 0.0) and all(not m.dyneval_stats_get(k).any() for k in want)
    same_bits(m.get_params(), theta, 'theta')


# ----------------------------------------------------------------------------- against fp64
def against_fp64(label, got, r64, r32, lengths, first):
    T = got['logprob'].shape[1]
    mask = (np.arange(T)[None, :] < np.asarray(lengths)[:, None]) & (np.arange(len(lengths))[:, None] >= first)
    e32_lp = np.abs(r32['logprob'] - r64['logprob'])[mask].max()
    err_lp = np.abs(got['logprob'].astype(np.float64) - r64['logprob'])[mask]
    bound_lp = np.maximum(NLL_RTOL * np.abs(r64['logprob'][mask]), 8 * e32_lp)
    nll_err = abs(got['nll'] - r64['nll']) / abs(r64['nll'])
    print('DYN64|%s|nll %.3g (fp32 %.3g)|logprob %.3g (e32 %.3g)' % (label, nll_err, abs(r32['nll'] - r64['nll']) / abs(r64['nll']), err_lp.max(), e32_lp))
    failures = []
    if not nll_err <= NLL_RTOL:
        failures.append('out_nll %.9g against %.9g' % (got['nll'], r64['nll']))
    if (err_lp > bound_lp).any():
        failures.append('%d log-probs outside the bound (worst %.3g)' % (int((err_lp > bound_lp).sum()), err_lp.max()))
    for k in sorted(r64['theta_l']):
        e32 = rel_max(r32['theta_l'][k], r64['theta_l'][k])
        err = rel_max(got['theta_l'][k], r64['theta_l'][k])
        print('DYN64|%s|%s|%.3g|e32 %.3g' % (label, k, err, e32))
        if not err <= max(REL_MAX, 8 * e32):
            failures.append('theta_l %s: %.3g (e32 %.3g)' % (k, err, e32))
    return failures


FP64_CASES = [(0, 'sgd', 0.02, MR.MAX_GRAD_NORM, 3, 2), (0, 'rms', 0.02, MR.MAX_GRAD_NORM_INACTIVE, 7, 1), (0, 'sgd', 0.0, MR.MAX_GRAD_NORM, 1, 'one'),
              (1, 'rms', 0.02, MR.MAX_GRAD_NORM, 6, 2), (2, 'sgd', 1.0, MR.MAX_GRAD_NORM_INACTIVE, 3, 'all'),
              (3, 'rms', 0.02, MR.MAX_GRAD_NORM, 3, 'all'), (4, 'sgd', 0.02, MR.MAX_GRAD_NORM, 3, 'all'), (5, 'rms', 0.02, MR.MAX_GRAD_NORM, 3, 'all')]


@pytest.mark.parametrize('idx,rule,decay,clip,seg,rows_per_step', FP64_CASES, ids=str)
def test_stream_against_fp64(idx, rule, decay, clip, seg, rows_per_step):
    cfg, theta, tokens, lengths = case(idx)
    R, first = ROWS[idx]
    adapt_reported = True
    if rows_per_step == 'one':      # seg_len 1: two rows, one per block, lengths (3, T): three live windows, then one unadapted window
        tokens, lengths, R, first, rows_per_step, adapt_reported = tokens[:2], np.array([3, cfg['max_len']], np.int32), 2, 1, 1, False
    elif idx == 0 and rows_per_step == 2:
        # lengths (2, 3 | T | 3), first_reported = 3 inside the grid's block (2, 4): the first block's windows [3, 6) and [6, 7) are
        # empty and skipped, the second walks all three, the reported row one: five updates
        tokens, lengths, R, first = tokens[:4], np.array([2, 3, cfg['max_len'], 3], np.int32), 4, 3
    P = R if rows_per_step == 'all' else rows_per_step
    stats = stats_for(theta)
    lr = SGD_LR if rule == 'sgd' else RMS_LR
    dcfg = dict(rule=rule, seg_len=seg, rows_per_step=P, lr=lr, decay=decay, eps=1e-3, clip_norm=clip, adapt_reported=adapt_reported)
    ref_cfg = D.dyn_config(rule=D.RMS if rule == 'rms' else D.SGD, seg_len=seg, rows_per_step=P, lr=lr, decay=decay, eps=1e-3, clip_norm=clip,
                           adapt_reported=adapt_reported)
    r64 = D.stream(MR.f64(theta), tokens, lengths, cfg, ref_cfg, first, stats=stats)
    r32 = D.stream(theta, tokens, lengths, cfg, ref_cfg, first, stats=stats)
    assert 1 <= len(r64['updates']) <= 6, len(r64['updates'])
    m = handle(cfg, theta, R, stats)
    got = score(m, dcfg, tokens, lengths, first)
    label = '%d|%s|d%g|c%g|S%d|P%d' % (idx, rule, decay, clip, seg, P)
    failures = against_fp64(label, got, r64, r32, lengths, first)
    assert not failures, '%s: %s' % (label, '; '.join(failures))
    if cfg['hidden_size'] >= 512:
        st = m.stats()
        assert st['xcd_launches'] + st['persistent_launches'] > 0
    assert m.stats()['timeouts'] == 0


# ----------------------------------------------------------------------------- the forced time-out
def test_timed_out_chain_repeats_the_whole_call():
    idx = 3
    cfg, theta, tokens, lengths = case(idx)
    R, first = ROWS[idx]
    stats = stats_for(theta)
    dcfg = dict(rule='rms', seg_len=3, rows_per_step=R, lr=RMS_LR, decay=0.02, eps=1e-3, clip_norm=MR.MAX_GRAD_NORM)
    ref_cfg = D.dyn_config(rule=D.RMS, seg_len=3, rows_per_step=R, lr=RMS_LR, decay=0.02, eps=1e-3, clip_norm=MR.MAX_GRAD_NORM)
    r64 = D.stream(MR.f64(theta), tokens, lengths, cfg, ref_cfg, first, stats=stats)
    r32 = D.stream(theta, tokens, lengths, cfg, ref_cfg, first, stats=stats)
    m = handle(cfg, theta, R, stats)
    m.forward_backward(tokens[None, :first], tokens[None, first:])
    st = m.stats()
    assert st['xcd_launches'] + st['persistent_launches'] > 0 and st['timeouts'] == 0 and st['persistent_path']
    m.debug_set('chain_spin_limit', 0)          # tests/test_maml_paths.py's knob: the persistent kernels give up at their first wait
    got = score(m, dcfg, tokens, lengths, first)                  # theta is back bitwise (score checks the whole state)
    st = m.stats()
    assert st['timeouts'] == 1 and not st['persistent_path']
    failures = against_fp64('timeout', got, r64, r32, lengths, first)
    assert not failures, '; '.join(failures)
    b = handle(cfg, theta, R, stats)
    b.debug_set('persistent', 0)                # what the repeat runs on
    want = score(b, dcfg, tokens, lengths, first)
    assert np.array_equal(bits(got['logprob']), bits(want['logprob']))
    same_bits(got['theta_l'], want['theta_l'], 'theta_l of the repeated call')


# ----------------------------------------------------------------------------- the plugin
def test_plugin_on_the_golden_lyrics(tmp_path, golden_dir):
    from conftest import ROOT
    from data.episode import load_sampler_from_config
    from models.dyneval_lstm import DynEvalLSTM
    from models.lstm_baseline import LSTMBaseline
    from test_masked_cpu import K, Q, T, _dataset, _raw_tree
    from test_train_entry import LOOP
    shipped = yaml.safe_load(open(os.path.join(ROOT, 'few-shot-music-generation_amd', 'src', 'config', 'dyneval_lstm.yaml')))
    root = _raw_tree(tmp_path, golden_dir)
    _dataset(root)[0].metadata.close()
    full = dict(LOOP, name='dyneval_lstm', model_module_name=shipped['model_module_name'], model_class_name=shipped['model_class_name'],
                n_decay=10000, lr=5e-3, max_grad_norm=5, embedding_size=32, hidden_size=40, n_layers=1, dataset='lyrics', dataset_path=root,
                splits=['train', 'val', 'test'], max_len=T, query_size=Q, support_size=K, seed=1234, split='train', dyneval_lengths=True)
    sampler = load_sampler_from_config(dict(full))
    full['input_size'] = sampler.get_num_unique_words()
    eps = [sampler.get_episode() for _ in range(3)]
    assert sum(int((e.support_len < T).sum() + (e.query_len < T).sum()) for e in eps) > 0
    p = DynEvalLSTM(dict(full, dyneval_rule='rms', dyneval_lr=1e-3, dyneval_decay=0.02, dyneval_seg_len=4, dyneval_rows_per_step=2, dyneval_clip=5.0))
    p.recover_or_init('')
    assert p.collect_stats(eps[:2]) == 2
    count, mean_rms = p.engine.dyneval_stats_info()
    assert count == 2 and mean_rms > 0
    nll = p.eval(eps[2])
    assert np.isfinite(nll) and nll > 0
    # saved and restored next to the native checkpoint
    p.save(str(tmp_path / 'ck'))
    q = DynEvalLSTM(dict(full, dyneval_rule='rms', dyneval_lr=1e-3, dyneval_decay=0.02, dyneval_seg_len=4, dyneval_rows_per_step=2, dyneval_clip=5.0))
    q.recover_or_init(str(tmp_path / 'ck'))
    assert q.engine.dyneval_stats_info() == (count, mean_rms)
    assert np.float32(q.eval(eps[2])) == np.float32(nll)
    # nothing adapts: the baseline's padding-masked NLL over the query rows
    still = DynEvalLSTM(dict(full, dyneval_lr=0.0, dyneval_decay=0.0, dyneval_seg_len=T))
    still.recover_or_init('')
    base = LSTMBaseline(dict(full, name='lstm_masked', model_class_name='LSTMBaseline', model_module_name='models.lstm_baseline', mask_padding=True))
    base.recover_or_init('')
    same_bits(base.engine.get_params(), still.engine.get_params(), 'the seeded parameters')
    got, want = still.eval(eps[2]), base.eval(eps[2])
    assert abs(got - want) <= NLL_RTOL * abs(want), (got, want)
    assert abs(nll - want) > NLL_RTOL * abs(want)                 # ... which the adapting plugin does not return
    toks = p.generate(eps[2].support[0], 5, n=2, seed=3, support_len=eps[2].support_len[0])
    assert toks.shape == (2, 5)
