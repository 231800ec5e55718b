"""The decode path's componentwise checks (tests/decode_ref.py) on the CPU alone: the fp32 stand-in that follows the kernels' order
passes every check on every shape of tests/test_gpu_decode_componentwise.py, each planted mistake fails on every shape where it
applies, the seeded parameters give gate pre-activations of spread 0.5 .. 2, and no comparison leaves an element out.  What the two
older checks (1e-4 at a picked token, 2e-5 norm-wise after twelve positions) make of each mistake is printed and recorded in
tests/COMPONENTWISE_DECODE.md.
"""
import numpy as np
import pytest

import decode_ref as D
from oracle import lstm_oracle as O

CELL_SHAPES = [(case, Hp) for case in D.CELL_CASES for Hp in case[4]]
CELL_PLANTS = ('drop_last_k', 'skip_partial_chunk', 'row_tile_alias', 'no_forget_bias', 'stale_x', 'pad_nonzero')
LP_PLANTS = ('drop_last_k', 'skip_partial_chunk', 'bias_tile', 'lse_over_ldl')
LP_SHAPES = D.LP_FULL + [(8, 16, V1) for V1, _ in D.LP_WIDE]

_CELLS = {}


def _cell_id(shape):
    return '%s-Hp%d' % (shape[0][0], shape[1])


def cell_setup(shape, R=D.CELL_ROWS):
    """parameters, inputs and the stand-in's step of one shape, computed once for the module and left unchanged"""
    key = (_cell_id(shape), R)
    if key not in _CELLS:
        (_, E, H, L, _), Hp = shape
        cfg = D.config(E, H, L, D.CELL_V)
        params = D.seeded_params(cfg)
        tok, h, c = D.seeded_state(cfg, R)
        h1, c1 = D.StandIn(params, cfg, Hp).cell(tok, h, c)
        _CELLS[key] = (cfg, params, tok, h, c, h1, c1)
    return _CELLS[key]


def test_the_shapes_reach_what_they_are_for():
    m = {case[0]: [(D.round_up(case[1], 16) // 16, Hp // 16) for Hp in case[4]] for case in D.CELL_CASES}
    assert m['E8-H16-L1'] == [(1, 1)]
    assert m['E20-H21-L2'] == [(2, 2)] and 21 % 4 != 0
    assert all(mx == D.GEN_CH for mx, _ in m['E250-H200-L1'])                      # exactly one register chunk in the x segment
    assert all(mx == 17 and mh > D.GEN_CH and mh % D.GEN_CH for mx, mh in m['E260-H260-L1'])      # a full chunk plus a partial one
    assert m['E16-H512-L1'] == [(1, 32)] and m['E16-H1024-L2'] == [(1, 64)]
    # rows: nrt = 1 .. 4 and a partial last block behind one and two full ones
    nrt = lambda R: [min(4, (R - r0 + 15) // 16) for r0 in range(0, R, D.GEN_ROWS)]
    assert [nrt(R) for R in D.ROW_COUNTS] == [[1], [1], [1], [2], [3], [4], [4], [4, 1], [4, 4, 1]]
    # the staging switch is a fact of V1
    assert [D.staged(V1) for V1, _ in D.LP_WIDE] == [s for _, s in D.LP_WIDE] == [True, True, False, False]


def test_checked_columns_hold_every_edge():
    for V1, _ in D.LP_WIDE:
        cols = D.checked_columns(V1)
        assert cols.size == D.MAX_CHECKED and len(set(cols.tolist())) == cols.size and cols.min() == 0 and cols.max() == V1 - 1
        have = set(cols.tolist())
        want = set(range(17)) | set(range(V1 - 17, V1)) | set(range(32760, min(V1, 32776)))
        for edge in range(D.SWEEP, V1 + 9, D.SWEEP):
            want |= set(v for v in range(edge - 8, edge + 9) if v < V1)
        assert want <= have and len(have - want) > 0          # and seeded random ones for the rest
    assert np.array_equal(D.checked_columns(98), np.arange(98))


@pytest.mark.parametrize('shape', CELL_SHAPES, ids=_cell_id)
def test_seeded_parameters_give_unsaturated_gates(shape):
    cfg, params, tok, h, c, h1, c1 = cell_setup(shape)
    res = D.check_cell(params, cfg, tok, h, c, h1, c1)
    print(_cell_id(shape), 'spread of the fp64 pre-activations per layer', res['z_std'])
    assert all(0.5 <= s <= 2.0 for s in res['z_std']), res['z_std']
    # the recurrent part matters: without h the pre-activations move by more than a tenth of their spread
    d = O.model_dims(cfg)
    x = params['embedding'][tok].astype(np.float64)
    K = params['kernel_0'].astype(np.float64)
    zh = h[0].astype(np.float64).dot(K[d['E']:])
    assert zh.std() >= 0.1 * res['z_std'][0]
    # the three edge tokens are read
    assert {0, d['V1'] - 2, d['V1'] - 1} <= set(tok.tolist()) and len(set(tok.tolist())) == len(tok)
    assert np.abs(h).max() < 1 and np.abs(c).max() < 2 and np.abs(c).max() > 1


@pytest.mark.parametrize('shape', CELL_SHAPES, ids=_cell_id)
def test_stand_in_passes_and_no_element_is_left_out(shape):
    cfg, params, tok, h, c, h1, c1 = cell_setup(shape)
    d = O.model_dims(cfg)
    Hp = shape[1]
    res = D.check_cell(params, cfg, tok, h, c, h1, c1)
    D.report(_cell_id(shape), res)
    assert D.passed(res)
    for f in D.FAMILIES:
        assert res[f]['n'] == d['L'] * D.CELL_ROWS * Hp and res[f]['n_zero'] == d['L'] * D.CELL_ROWS * (Hp - d['H'])
        assert D.U <= res[f]['e32'] < 1e-5
    # what the device returns (H units a row) is compared whole as well
    res = D.check_cell(params, cfg, tok, h, c, h1[:, :, :d['H']], c1[:, :, :d['H']])
    assert D.passed(res) and all(res[f]['n'] == h.size and res[f]['n_zero'] == 0 for f in D.FAMILIES)


@pytest.mark.parametrize('R', D.ROW_COUNTS)
def test_stand_in_passes_at_every_row_count(R):
    shape = (D.ROWS_CASE, D.ROWS_CASE[4][0])
    for copies in (False, True):
        (_, E, H, L, _), Hp = shape
        cfg = D.config(E, H, L, D.CELL_V)
        params = D.seeded_params(cfg)
        tok, h, c = D.seeded_state(cfg, R, copies=copies)
        h1, c1 = D.StandIn(params, cfg, Hp).cell(tok, h, c)
        res = D.check_cell(params, cfg, tok, h, c, h1, c1)
        assert D.passed(res) and res['h']['n'] == L * R * Hp
        if copies:
            assert len(set(tok.tolist())) == 1 and all(np.array_equal(a[:, r], a[:, 0]) for a in (h, c, h1, c1) for r in range(R))
        else:
            assert len(set(tok.tolist())) == R


@pytest.mark.parametrize('plant', CELL_PLANTS)
@pytest.mark.parametrize('shape', CELL_SHAPES, ids=_cell_id)
def test_planted_mistake_in_the_cell_fails(shape, plant):
    cfg, params, tok, h, c, h1, c1 = cell_setup(shape)
    sim = D.StandIn(params, cfg, shape[1], plant)
    if not sim.applies():
        # nothing of this shape is touched: the same bits as the clean stand-in (checked where the step is cheap)
        if shape[1] <= 64:
            p1, q1 = sim.cell(tok, h, c)
            assert np.array_equal(p1, h1) and np.array_equal(q1, c1)
        return
    p1, q1 = sim.cell(tok, h, c)
    res = D.check_cell(params, cfg, tok, h, c, p1, q1)
    print(_cell_id(shape), plant, 'h %.3g x e32 (%d elements over M), c %.3g x e32 (%d)' %
          (res['h']['ratio'], res['h']['fails'], res['c']['ratio'], res['c']['fails']))
    assert not D.passed(res)
    assert max(res['h']['ratio'], res['c']['ratio']) >= 10 * D.M         # missed by a factor of ten at least, not by a hair
    if plant == 'pad_nonzero':
        # only the exact-zero comparison sees it, and the device's get() (H units a row) cannot
        assert res['h']['fails'] == D.CELL_ROWS * O.model_dims(cfg)['L'] and res['c']['fails'] == 0
        assert D.passed(D.check_cell(params, cfg, tok, h, c, p1[:, :, :shape[0][2]], q1[:, :, :shape[0][2]]))
    if plant == 'row_tile_alias':
        assert res['h']['fails'] > 0 and res['h']['where'][1] >= 16


def test_every_cell_plant_applies_somewhere():
    for plant in CELL_PLANTS:
        n = 0
        for case, Hp in CELL_SHAPES:
            cfg = D.config(case[1], case[2], case[3], D.CELL_V)
            n += D.StandIn(D.seeded_params(cfg), cfg, Hp, plant).applies()
        assert n >= 2, plant


_LPS = {}


def lp_setup(E, H, V1):
    key = (E, H, V1)
    if key not in _LPS:
        cfg = D.config(E, H, 1, V1 - 1)
        params = D.seeded_params(cfg)
        tok, h, c = D.seeded_state(cfg, 1)
        h1, _ = D.StandIn(params, cfg, D.round_up(H, 16)).cell(tok, h, c)
        _LPS[key] = (cfg, params, h1[-1, 0, :H])
    return _LPS[key]


@pytest.mark.parametrize('shape', LP_SHAPES, ids=lambda s: 'H%d-V%d' % (s[1], s[2]))
def test_stand_in_logit_rows_pass_and_planted_mistakes_fail(shape):
    E, H, V1 = shape
    cfg, params, h_top = lp_setup(*shape)
    cols = None if V1 <= 1025 else D.checked_columns(V1)
    Hp = D.round_up(H, 16)
    res = dict(lp=D.check_lp(params, h_top, D.StandIn(params, cfg, Hp).logprobs(h_top, cols), cols))
    D.report('H%d-V%d' % (H, V1), res)
    assert D.passed(res) and res['lp']['n'] == (V1 if cols is None else D.MAX_CHECKED) and ('sum' in res['lp']) == (cols is None)
    assert D.U <= res['lp']['e32'] < 1e-5
    for plant in LP_PLANTS:
        sim = D.StandIn(params, cfg, Hp, plant)
        if not sim.applies(lp=True):          # one column tile, ldl == V1, or no partial chunk: the same bits as the clean stand-in
            assert np.array_equal(sim.logprobs(h_top, cols), D.StandIn(params, cfg, Hp).logprobs(h_top, cols))
            continue
        bad = dict(lp=D.check_lp(params, h_top, sim.logprobs(h_top, cols), cols))
        print('H%d-V%d' % (H, V1), plant, 'lp %.3g x e32 (%d elements over M)' % (bad['lp']['ratio'], bad['lp']['fails']))
        assert not D.passed(bad) and bad['lp']['ratio'] >= 10 * D.M, plant
        if plant == 'bias_tile':
            assert bad['lp']['where'][0] >= 16 * ((V1 - 1) // 16) or bad['lp']['fails'] > 1


def test_partial_chunk_plant_on_the_logits_at_m_17():
    """no logit-row shape of the GPU test has a hidden width with m = 17 and a whole row; the plant is shown on one here"""
    cfg = D.config(8, 272, 1, 97)
    params = D.seeded_params(cfg)
    h_top = D.seeded_state(cfg, 1)[1][0, 0] * np.float32(0.5)
    assert D.passed(dict(lp=D.check_lp(params, h_top, D.StandIn(params, cfg, 272).logprobs(h_top))))
    sim = D.StandIn(params, cfg, 272, 'skip_partial_chunk')
    assert sim.applies(lp=True) and not D.passed(dict(lp=D.check_lp(params, h_top, sim.logprobs(h_top))))


def test_a_wrong_column_nobody_picks_is_seen():
    """what gen_ref.check_margins cannot see: the least likely column of a row off by 5e-5, half of its 1e-4"""
    cfg, params, h_top = lp_setup(8, 16, 98)
    lp = D.StandIn(params, cfg, 16).logprobs(h_top)
    v = int(np.argmin(lp))
    lp[v] += np.float32(5e-5)
    res = D.check_lp(params, h_top, lp)
    assert res['fails'] == 1 and res['where'] == (v,)


E5_SHAPES = {'h24': dict(input_size=97, embedding_size=12, hidden_size=24), 'h200x2': dict(input_size=97, embedding_size=12, hidden_size=200, n_layers=2)}


@pytest.mark.parametrize('name', sorted(E5_SHAPES))
def test_what_the_older_checks_make_of_the_planted_mistakes(name):
    """recorded in tests/COMPONENTWISE_DECODE.md; the clean stand-in passes both older checks"""
    clean = D.older_checks_see(None, E5_SHAPES[name])
    print('%-7s %-20s norm-wise %.2e  margin %.2e' % (name, 'clean', clean['worst_norm'], clean['worst_margin']))
    assert not clean['norm'] and not clean['margin']
    for plant in D.PLANTS:
        r = D.older_checks_see(plant, E5_SHAPES[name])
        print('%-7s %-20s norm-wise %.2e (%s)  margin %.2e (%s)%s' %
              (name, plant, r['worst_norm'], 'seen' if r['norm'] else 'not seen', r['worst_margin'],
               'seen' if r['margin'] else 'not seen', '' if r['applies'] else '  [the shape never reaches it]'))
        assert np.isfinite(r['worst_norm']) and np.isfinite(r['worst_margin'])
