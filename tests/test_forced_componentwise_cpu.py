"""The references of tests/test_gpu_forced_componentwise.py, on the CPU alone (tests/backward_ref.py has the case lists).

  * every shape of the lists builds its fp64 / fp32 reference pair, every e32 is a number, no family is vacuous;
  * the restated dispatch (backward_ref.expected_dispatch) picks, at every case, the kernel family the case is there for -- so
    a change of a list or of the rule that empties a case shows here, before any GPU run;
  * planted mistakes of the kind a recurrence kernel can make.  Two pass the norm-wise bars of tests/test_gpu_parity.py and miss
    the elementwise bound M * e32 by factors of tens to hundreds of thousands: a zeroed gate block of dz, a k-group left out of
    dh's recurrent sum.  Two were tried and are recorded, not kept: stale units of the last row of hs (these episodes move every
    unit by per cent from step to step: the norm-wise bar sees them too) and a dropped low bf16 plane of h_{t-1} (it lands AT the
    bound, 0.8 .. 1.2 of it).  The factors are in tests/COMPONENTWISE.md.

Every planted mistake is applied to the fp64 reference's own tensors: what is tested is the measure, not a kernel.
"""
import numpy as np
import pytest

import backward_ref as R
from conftest import small_config
from gpu_utils import rel_max
from oracle import lstm_oracle as O

M = 8                       # the device's bound is M * e32 (tests/test_gpu_componentwise.py)
HS_BAR, GRAD_BAR = 2e-5, 2e-4          # the norm-wise bars of tests/test_gpu_parity.py: hs / cs / logits, gradients

_REFS = {}


def reference(case):
    shape = R.forced_shape(case)
    key = R.shape_id(shape)
    if key not in _REFS:
        over, N, K, Q, seed = shape
        cfg = small_config(**over)
        sup, qry = R.episode(cfg, N, K, Q, seed)
        X, Y = O.train_xy(sup, qry, cfg['input_size'])
        _REFS[key] = (cfg, R.Reference(O.glorot_init(cfg, 0), X, Y, cfg))
    return _REFS[key]


ALL_CASES = R.FORCED_CASES + [R.FORCED_RECOVERY]
UNIQUE_SHAPES = list({R.shape_id(R.forced_shape(c)): c for c in ALL_CASES}.values())


@pytest.mark.parametrize('case', UNIQUE_SHAPES, ids=lambda c: R.shape_id(R.forced_shape(c)))
def test_reference_of_every_forced_shape_is_a_yardstick(case):
    cfg, ref = reference(case)          # (Reference asserts the fp32 pass's exact zeros wherever S == 0 itself)
    over, N, K, Q, seed = R.forced_shape(case)
    assert ref.X.shape == (N * (K + Q), cfg['max_len'])
    assert sorted(ref.e32) == sorted(R.FAMILIES)
    for fam, e in ref.e32.items():
        # plain fp32 arithmetic (the band of tests/test_componentwise_cpu.py): a family inflated the way "all lengths 1" inflates
        # softmax_w / kernel / bias (tests/COMPONENTWISE.md) would leave it
        assert np.isfinite(e) and 1e-8 < e < 1e-4, (fam, e)
        # (1 row x 3 steps gave kernel 1.4e-4 at hidden 512, 4 stacked rows 2.9e-5, 6 rows 4.1e-5; the shapes as they are now 1e-6 .. 7e-6.
        # e32 is a maximum over up to 12.6 M elements and moves with the host's BLAS: 4.9e-6 and 6.8e-6 for one shape on two hosts)
        if fam in ('softmax_w', 'kernel', 'bias'):
            assert e < 2e-5, (fam, e)
    for (fam, layer), ref_t in ref.t.items():
        assert not ref.failures(fam, layer, ref_t, M).any()
        if fam in R.COMPONENTWISE:      # not vacuous: something is held to a bound, not only to zero
            assert (R.scale_of(ref.full, fam, layer) > 0).any(), fam
        else:
            assert (np.abs(ref_t).max(axis=R.SLICE_AXES[fam]) > 0).any(), fam
    # two recurrent steps at least: h_{t-1} and the dc carry are live
    assert cfg['max_len'] >= 3
    assert np.abs(ref.t[('hs', 0)][2]).max() > 0 and np.abs(ref.t[('dz', 0)][:, 0]).max() > 0


def test_case_ids_are_unique():
    ids = [R.forced_id(c) for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    assert R.CW_SHAPES[0] == (dict(), 2, 2, 1, 3) and len(R.CW_SHAPES) == 14          # untouched


def _d(case, **kw):
    env, over, N, K, Q, seed = case
    return R.expected_dispatch(small_config(**over), N * (K + Q), env, **kw)


def test_restated_dispatch_picks_the_family_each_case_is_there_for():
    """the rule of backward_ref.expected_dispatch at every case -- what the GPU test asserts the device's counters against"""
    for c in R.FORCED_ROW_EDGES:
        d, B, H = _d(c), c[2] * (c[3] + c[4]), c[1]['hidden_size']
        T = c[1]['max_len']
        assert d['Hp'] == H
        if H == 512:
            # 1 / 2 / 4 / 4 row groups up to 32 / 64 / 96 / 128 rows; above: 9 row tiles -- more than k_lstm_fwd_chain's 921 blocks,
            # k_lstm_fwd_chain_rt's 4 row tiles and k_lstm_bwd_rs's 230 blocks take -- so one launch per time step, not a persistent one
            want = (2, 0, 0) if B <= 128 else (0, 0, 2 * T)
            assert d['xcd_bx3'] == (64 < B <= 128)
        elif H == 1024:
            # the pair kernels up to 64 rows, bf16-split from three row groups (33 rows) on; 65 rows are 5 row tiles: per step
            want = (2, 0, 0) if B <= 64 else (0, 0, 2 * T)
            assert d['xcd_bx3'] == (B >= 33)           # (at 65 rows the format is what select_xcd_format left; no XCD-local kernel runs)
        elif H == 256:
            want = (2, 0, 0) if B <= 128 else (0, 2, 0)          # slice kernels, then k_lstm_fwd_chain<4> + k_lstm_bwd_rs<2>
        elif H == 128:
            want = (0, 2, 0)
        else:
            want = (0, 0, 2 * T)
            assert (d['fwd'], B) == ('patch', 70)
        assert (d['xcd_launches'], d['persistent_launches'], d['step_launches']) == want, R.forced_id(c)
        assert not d['xov']
    for c in R.FORCED_PER_STEP:
        d = _d(c)
        T, L = c[1]['max_len'], c[1]['n_layers']
        assert (d['xcd_launches'], d['persistent_launches'], d['step_launches']) == (0, 0, 2 * T * L) and not d['xcd_bx3']
        assert d['Hp'] == (256 if c[1]['hidden_size'] == 200 else c[1]['hidden_size'])
        assert d['fwd'] == ('patch' if c[2] * (c[3] + c[4]) >= 49 else 'step')
    kernels = [(_d(c)['fwd'], _d(c)['bwd']) for c in R.FORCED_COLUMN_SPLIT]
    assert kernels == [('chain', 'rs'), ('chain', 'rs'), ('chain', 'rs'), ('chain', 'rs'),                # FSMG_XCD=0: 256 and 512, 45 and 100 rows (7 row tiles: 896 of 921 blocks at 512)
                       ('chain', 'rs'), ('chain_rt', 'rs'), ('xcd', 'rs'), ('xcd', 'rs'),                 # FSMG_XCD_PAIR=0 / 1: 4 (stacked) and 45 rows
                       ('chain_rt', 'rs'), ('chain_rt', 'chain')], kernels                                  # FSMG_FWD_RT=1
    assert [_d(c)['xcd_bx3'] for c in R.FORCED_XCD_ARITH] == [True, True, False, True, True, True]
    assert all((_d(c)['fwd'], _d(c)['bwd']) == ('xcd', 'xcd') for c in R.FORCED_XCD_ARITH + R.FORCED_XOV)
    got = [(c[0]['FSMG_XCD_OVERLAP'], _d(c)['xov_fwd'], _d(c)['xov_bwd'], _d(c)['dk_tail'], _d(c)['xcd_bx3']) for c in R.FORCED_XOV]
    assert got == [('1', True, False, False, True), ('0', False, False, False, False),       # 45 x 6: the forward pair alone
                   ('1', False, False, False, True), ('0', False, False, False, True),       # 100 x 6: seven XCDs of chain -- the order declines
                   ('1', True, True, False, True), ('0', False, False, False, True),         # 80 x 7: both pairs, dK in its own launch (Ep = 16)
                   ('1', True, True, True, True), ('0', False, False, False, False)], got     # 45 x 46, E = 250: both pairs + the joint launch
    d = _d(R.FORCED_RECOVERY)
    assert (d['fwd'], d['bwd'], d['xcd_bx3']) == ('xcd', 'xcd', False)
    d = _d(R.FORCED_RECOVERY, persist_now=False)
    assert (d['xcd_launches'], d['persistent_launches'], d['step_launches']) == (0, 0, 8)


# ----------------------------------------------------------------------------- planted mistakes
def forward_restated(ref, cfg, round_h_bits=0):
    """layer 0 of oracle.lstm_oracle.forward in fp64, statement for statement; round_h_bits: h_{t-1} enters the recurrent product
    rounded to that many significant bits (16: a bf16 split whose low plane is dropped) -> hs, cs [T+1, B, H]"""
    p, X = ref.params, ref.X
    H, T = cfg['hidden_size'], cfg['max_len']
    B = X.shape[0]
    K, b = p['kernel_0'], p['bias_0']
    layer_in = p['embedding'][X]
    n_in = layer_in.shape[2]
    zx = layer_in.reshape(B * T, n_in).dot(K[:n_in]).reshape(B, T, 4 * H) + b
    h, c = np.zeros((B, H)), np.zeros((B, H))
    hs, cs = np.zeros((T + 1, B, H)), np.zeros((T + 1, B, H))
    for t in range(T):
        hin = h
        if round_h_bits:
            m, e = np.frexp(h)
            hin = np.ldexp(np.round(m * 2.0 ** round_h_bits) / 2.0 ** round_h_bits, e)
        z = zx[:, t] + hin.dot(K[n_in:])
        si, tj = O._sigmoid(z[:, :H]), np.tanh(z[:, H:2 * H])
        sf, so = O._sigmoid(z[:, 2 * H:3 * H] + O.FORGET_BIAS), O._sigmoid(z[:, 3 * H:])
        c = c * sf + si * tj
        h = np.tanh(c) * so
        hs[t + 1], cs[t + 1] = h, c
    return hs, cs


def bptt_restated(ref, cfg, zero_dz=None, drop_k=None):
    """layer 0's loop of backward_ref.backward_full in fp64, statement for statement -> dz [B, T, 4H].
    zero_dz = (b, t, gate): that gate block of dz is stored as zeros (and what it would have sent to step t - 1 is lost with it);
    drop_k = (b, t, cols): dh_{t} of row b is summed without the columns `cols` of dz_{t+1}"""
    p, lay = ref.params, ref.cache['layers'][0]
    H, T = cfg['hidden_size'], cfg['max_len']
    B = ref.X.shape[0]
    Kh = p['kernel_0'][lay['x'].shape[2]:]
    dtop = ref.full['dh'].reshape(B, T, H)
    dz_all = np.zeros((B, T, 4 * H))
    dh_rec, dc = np.zeros((B, H)), np.zeros((B, H))
    for t in reversed(range(T)):
        si, tj, sf, so = lay['gates'][t]
        c_t, c_prev = lay['cs'][t + 1], lay['cs'][t]
        tc = np.tanh(c_t)
        dht = dtop[:, t] + dh_rec
        do = dht * tc * so * (1.0 - so)
        dc = dc + dht * so * (1.0 - tc * tc)
        di = dc * tj * si * (1.0 - si)
        dj = dc * si * (1.0 - tj * tj)
        df = dc * c_prev * sf * (1.0 - sf)
        dz = np.concatenate([di, dj, df, do], axis=1)
        if zero_dz is not None and zero_dz[1] == t:
            dz[zero_dz[0], zero_dz[2] * H:(zero_dz[2] + 1) * H] = 0.0
        dz_all[:, t] = dz
        dh_rec = dz.dot(Kh.T)
        if drop_k is not None and drop_k[1] == t - 1:
            dh_rec[drop_k[0]] -= dz[drop_k[0], drop_k[2]].dot(Kh[:, drop_k[2]].T)
        dc = dc * sf
    return dz_all


def gradients_of(ref, cfg, dz):
    """kernel_0, bias_0, dx and the embedding gradient that a pass with this dz would produce (backward_full's statements)"""
    lay = ref.cache['layers'][0]
    B, T, H = ref.X.shape[0], cfg['max_len'], cfg['hidden_size']
    n = B * T
    dzf = dz.reshape(n, 4 * H)
    n_in = lay['x'].shape[2]
    hprev = np.transpose(lay['hs'][:-1], (1, 0, 2)).reshape(n, H)
    kernel = np.concatenate([lay['x'].reshape(n, n_in).T.dot(dzf), hprev.T.dot(dzf)], axis=0)
    dx = dzf.dot(ref.params['kernel_0'][:n_in].T)
    emb = np.zeros_like(ref.params['embedding'])
    np.add.at(emb, ref.X.reshape(n), dx)
    return dict(kernel=kernel, bias=dzf.sum(axis=0), dx=dx, embedding=emb)


# 45 rows (a partial row tile: row 44 is its last) at hidden 512 over 6 steps, and 49 rows at hidden 128 over 3
PLANT_CASES = [R.FORCED_XOV[0], R.FORCED_ROW_EDGES[29]]
PLANT_IDS = [R.shape_id(R.forced_shape(c)) for c in PLANT_CASES]


def test_restatements_of_the_planting_helpers_are_the_reference_bit_for_bit():
    assert PLANT_IDS == ['E16-H512-I60-M6-N1-5x5x4', 'E16-H128-I60-M3-N1-7x4x3']
    for case in PLANT_CASES:
        cfg, ref = reference(case)
        hs, cs = forward_restated(ref, cfg)
        np.testing.assert_array_equal(hs, ref.t[('hs', 0)])
        np.testing.assert_array_equal(cs, ref.t[('cs', 0)])
        dz = bptt_restated(ref, cfg)
        B, T, H = ref.X.shape[0], cfg['max_len'], cfg['hidden_size']
        np.testing.assert_array_equal(dz.reshape(B, T, 4, H), ref.t[('dz', 0)])
        g = gradients_of(ref, cfg, dz)
        for fam in ('kernel', 'bias'):
            np.testing.assert_array_equal(g[fam], ref.t[(fam, 0)])
        np.testing.assert_array_equal(g['dx'], ref.t[('dx', None)])
        np.testing.assert_array_equal(g['embedding'], ref.t[('embedding', None)])


def _report(name, case, bars, misses):
    """bars: {tensor: rel_max}, all inside the norm-wise bars; misses: {family: ratio over e32}, the worst at least M"""
    print('PLANT|%s|%s|%s|%s' % (name, R.shape_id(R.forced_shape(case)),
                                 ', '.join('%s %.1e' % kv for kv in sorted(bars.items())),
                                 ', '.join('%s %.1f' % (k, v / M) for k, v in sorted(misses.items()))))


@pytest.mark.parametrize('case', PLANT_CASES, ids=PLANT_IDS)
def test_stale_units_of_the_last_row_of_a_partial_row_tile_do_not_hide_from_either_check(case):
    """row B - 1 keeps its hs of step t - 1 at one step.  NOT a mistake only the elementwise bound sees: on these episodes every unit of
    the row moves from step to step -- even the unit block of 4 that moves least, at the step where it moves least, by 2 % .. 8 % of
    the tensor's largest |h| -- so the norm-wise bar of 2e-5 sees a stale row as well as the bound does.  Recorded, not kept."""
    cfg, ref = reference(case)
    hs = ref.t[('hs', 0)]
    b = hs.shape[1] - 1
    assert (b + 1) % 16 != 0                      # the last row tile is partial
    move = np.abs(hs[2:, b] - hs[1:-1, b])        # [T - 1, H]: what a stale store at step t = 1 .. T - 1 would get wrong
    blocks = move.reshape(move.shape[0], -1, 4).max(axis=2)
    t_blk, u = np.unravel_index(int(np.argmin(blocks)), blocks.shape)
    planted = hs.copy()
    planted[t_blk + 2, b, 4 * u:4 * u + 4] = hs[t_blk + 1, b, 4 * u:4 * u + 4]
    bar = rel_max(planted, hs)
    ratio, where = ref.ratio('hs', 0, planted)
    _report('stale hs, least-moving unit block', case, dict(hs=bar), dict(hs=ratio))
    assert bar > HS_BAR
    assert where == (t_blk + 2, b) and ref.failures('hs', 0, planted, M).sum() == 1 and ratio / M > 1000, (ratio, where)


@pytest.mark.parametrize('case', PLANT_CASES, ids=PLANT_IDS)
def test_dropped_low_plane_of_the_recurrent_input_is_seen(case):
    """h_{t-1} enters the recurrent product with 16 significant bits: two of the three bf16 planes of k_lstm_*_xcd16 / pair16"""
    cfg, ref = reference(case)
    hs, cs = forward_restated(ref, cfg, round_h_bits=16)
    bars = dict(hs=rel_max(hs, ref.t[('hs', 0)]), cs=rel_max(cs, ref.t[('cs', 0)]))
    assert all(0 < v < HS_BAR for v in bars.values()), bars
    misses = dict(hs=ref.ratio('hs', 0, hs)[0], cs=ref.ratio('cs', 0, cs)[0])
    _report('h_{t-1} with 16 significant bits', case, bars, misses)
    # NOT kept as a mistake the bound sees: it lands at 0.8 .. 1.2 of M * e32 (6.5 .. 9.6 x e32) -- eight fewer bits of h_{t-1} are an
    # error of 2^-17 |h| |K_h| per term, the size of the bound itself.  What holds on any host: it is several times what plain fp32
    # arithmetic does (e32), and far below what the norm-wise bar asks.
    assert min(misses.values()) > 2, misses
    # h_0 = 0 enters step 0 unrounded: h_1 is the reference's bit for bit, the first state that can differ is h_2
    assert np.array_equal(hs[:2], ref.t[('hs', 0)][:2]) and not np.array_equal(hs[2], ref.t[('hs', 0)][2])


def _grad_bars(ref, g):
    return dict(kernel=rel_max(g['kernel'], ref.t[('kernel', 0)]), bias=rel_max(g['bias'], ref.t[('bias', 0)]),
                embedding=rel_max(g['embedding'], ref.t[('embedding', None)]))


def _grad_misses(ref, cfg, dz, g):
    B, T, H = ref.X.shape[0], cfg['max_len'], cfg['hidden_size']
    out = dict(dz=ref.ratio('dz', 0, dz.reshape(B, T, 4, H))[0], dx=ref.ratio('dx', None, g['dx'])[0])
    for fam in ('kernel', 'bias'):
        out[fam] = ref.ratio(fam, 0, g[fam])[0]
    out['embedding'] = ref.ratio('embedding', None, g['embedding'])[0]
    return out


@pytest.mark.parametrize('case', PLANT_CASES, ids=PLANT_IDS)
def test_zeroed_gate_block_of_dz_is_seen(case):
    """dz of one gate block of the (t, b) row with the smallest |dz| is stored as zeros"""
    cfg, ref = reference(case)
    dz_ref = ref.t[('dz', 0)]                                       # [B, T, gate, H]
    size = np.abs(dz_ref).max(axis=3)
    size[size == 0] = np.inf
    b, t, gate = np.unravel_index(int(np.argmin(size)), size.shape)
    dz = bptt_restated(ref, cfg, zero_dz=(b, t, gate))
    g = gradients_of(ref, cfg, dz)
    bars = _grad_bars(ref, g)
    assert all(v < GRAD_BAR for v in bars.values()) and max(bars.values()) > 0, bars
    misses = _grad_misses(ref, cfg, dz, g)
    _report('zeroed gate block of dz', case, bars, misses)
    B, T, H = ref.X.shape[0], cfg['max_len'], cfg['hidden_size']
    bad = ref.failures('dz', 0, dz.reshape(B, T, 4, H), M)
    assert bad[b, t, gate] and misses['dz'] / M > 1, misses


@pytest.mark.parametrize('case', PLANT_CASES, ids=PLANT_IDS)
def test_k_group_left_out_of_the_recurrent_sum_of_dh_is_seen(case):
    """one k-group -- 16 packed gate columns: 4 units x 4 gates, the device's column order -- of dz_{t+1} is left out of dh_t of one
    row: the row, step and group whose share of dh_t is smallest relative to the row"""
    cfg, ref = reference(case)
    B, T, H = ref.X.shape[0], cfg['max_len'], cfg['hidden_size']
    Kh = ref.params['kernel_0'][cfg['embedding_size']:]
    dz_ref = ref.t[('dz', 0)]                                       # [B, T, gate, H]
    best = (np.inf, None)
    for u in range(0, H, 4):
        cols = np.concatenate([np.arange(g * H + u, g * H + u + 4) for g in range(4)])
        share = dz_ref.reshape(B, T, 4 * H)[:, 1:, cols].dot(Kh[:, cols].T)          # [B, T - 1, H]: what dh_t loses, t = 0 .. T - 2
        rel = np.abs(share).max(axis=2)
        rel[rel == 0] = np.inf
        i = np.unravel_index(int(np.argmin(rel)), rel.shape)
        if rel[i] < best[0]:
            best = (rel[i], (int(i[0]), int(i[1]), cols))
    dz = bptt_restated(ref, cfg, drop_k=best[1])
    assert not np.array_equal(dz, dz_ref.reshape(B, T, 4 * H))
    g = gradients_of(ref, cfg, dz)
    bars = _grad_bars(ref, g)
    assert all(v < GRAD_BAR for v in bars.values()), bars
    misses = _grad_misses(ref, cfg, dz, g)
    _report('k-group left out of dh', case, bars, misses)
    assert max(misses.values()) / M > 1, misses
