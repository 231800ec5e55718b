"""-m gpu: k_gen_cell, k_gen_logits and row_max_lse (csrc/decode.hip) against fp64 ELEMENT BY ELEMENT at their tile and K edges.

Every decode entry point advances through advance() (csrc/api_decode.hip), so these three are what fsmg_sample, fsmg_generate*,
fsmg_beam_search, fsmg_dstate_*, the cache-conditioned generators and the MAML twins compute with.  They are reached through the public
calls alone -- new_state, set, gather, feed, get -- with the technique, the measure and the bound M * e32 (M = 8) of tests/decode_ref.py:

  * one cell step in isolation: a seeded non-zero state and one pending token per row are set, one token is fed, the state is read
    back; layer l is held to one fp64 step from the device's own inputs (test_one_cell_step, test_row_counts);
  * a whole row of logits: the state is gathered to V1 copies of one row, row v is fed token v with log-probs, so the call returns
    z[v] - lse of one h for every v; all rows must then hold the same bits of h and c (test_full_logit_rows);
  * wide rows: 256 checked columns, the reference lse over all V1 (test_wide_logit_rows; staged up to 32 768 columns, unstaged above).

fsmg_dstate_get returns hidden_size units a row, so the pad units of the device's state are not visible here; the exact-zero rule for
them is exercised on the stand-in (tests/test_decode_componentwise_cpu.py).  Measured figures: tests/COMPONENTWISE_DECODE.md.
"""
import numpy as np
import pytest

import decode_ref as D
from gpu_utils import new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

assert D.M == 8               # the project's number: no case here gets another
_MODELS = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def seeded_model(E, H, L, V):
    """a handle whose parameters are the seeded fp32 ones bit for bit; the one configuration two tests share is kept for the module
    (no test changes a parameter), the others are closed by the garbage collector with their test"""
    key = (E, H, L, V)
    if key in _MODELS:
        return _MODELS[key]
    cfg = D.config(E, H, L, V)
    params = D.seeded_params(cfg)
    m = new_model(cfg, params)
    back = m.get_params()
    assert all(np.array_equal(bits(back[k]), bits(params[k])) for k in params)
    if (E, H, L) == D.ROWS_CASE[1:4]:
        _MODELS[key] = (m, cfg, params)
    return m, cfg, params


def one_step(m, tok, h, c):
    """set (h, c, pending token), feed one token without log-probs, get: the pending token is what the step reads"""
    R = tok.shape[0]
    st = m.new_state(R, history=4)
    st.set(h, c, ctx=tok[:, None], n_ctx=1)
    m.feed(st, np.zeros((R, 1), np.int32))
    got = st.get()
    st.close()
    assert got['n_ctx'] == 2 and got['ctx'][:, 0].tolist() == tok.tolist()
    return got['h'], got['c']


def assert_ok(label, res, m):
    D.report(label, res)
    assert m.stats()['timeouts'] == 0
    for f in ('c', 'h', 'lp'):
        if f in res:
            r = res[f]
            assert r['fails'] == 0, '%s %s: %d of %d elements over %d x e32, worst %.2f x e32 (e32 %.2e) at %s' % (
                label, f, r['fails'], r['n'], D.M, r['ratio'], r['e32'], r['where'])
            assert r.get('sum_ok', True), (label, r['sum'], r['sum_bound'])


@pytest.mark.parametrize('case', D.CELL_CASES, ids=D.cell_id)
def test_one_cell_step(case):
    name, E, H, L, hps = case
    m, cfg, params = seeded_model(E, H, L, D.CELL_V)
    dd = m.debug_dims()
    assert dd['Ep'] == D.round_up(E, 16) and dd['Hp'] in hps, dd
    mx, mh = dd['Ep'] // 16, dd['Hp'] // 16
    if name == 'E8-H16-L1':
        assert (mx, mh) == (1, 1)
    elif name == 'E20-H21-L2':
        assert (dd['Ep'], dd['Hp']) == (32, 32)
    elif name == 'E250-H200-L1':
        assert dd['Ep'] == 256 and mx == D.GEN_CH
    elif name == 'E260-H260-L1':
        assert dd['Ep'] == 272 and mx == 17 and mh > 16 and mh % 16 != 0
    else:
        assert mh == H // 16 and mh in (32, 64)
    tok, h, c = D.seeded_state(cfg, D.CELL_ROWS)
    h1, c1 = one_step(m, tok, h, c)
    res = D.check_cell(params, cfg, tok, h, c, h1, c1)
    assert all(res[f]['n'] == L * D.CELL_ROWS * H for f in D.FAMILIES)
    assert_ok('%s-Hp%d' % (name, dd['Hp']), res, m)


@pytest.mark.parametrize('R', D.ROW_COUNTS)
def test_row_counts(R):
    """nrt = 1 .. 4 row tiles and gridDim.y = 1 .. 3 with a partial last block, with distinct rows and as R copies of one row: the
    copies must come back as the same bits in every row"""
    name, E, H, L, hps = D.ROWS_CASE
    m, cfg, params = seeded_model(E, H, L, D.CELL_V)
    assert m.debug_dims()['Hp'] == hps[0]
    for copies in (False, True):
        tok, h, c = D.seeded_state(cfg, R, copies=copies)
        h1, c1 = one_step(m, tok, h, c)
        if copies:
            for a in (h1, c1):
                assert np.array_equal(bits(a), bits(np.repeat(a[:, :1], R, 1))), 'rows of one state differ'
        res = D.check_cell(params, cfg, tok, h, c, h1, c1)
        assert all(res[f]['n'] == L * R * H for f in D.FAMILIES)
        assert_ok('%s-R%d%s' % (name, R, '-copies' if copies else ''), res, m)


def logit_row(m, cfg, params, cols):
    """one seeded row, gathered to len(cols) copies, row v fed token cols[v] with log-probs -> the check of its cell step and of the
    log-probs at cols"""
    n = len(cols)
    tok, h, c = D.seeded_state(cfg, 1)
    src, dst = m.new_state(1, history=4), m.new_state(n, history=4)
    src.set(h, c, ctx=tok[:, None], n_ctx=1)
    dst.gather(src, np.zeros(n, np.int32))
    lp = m.feed(dst, np.asarray(cols, np.int32)[:, None], logprobs=True)[:, 0]
    got = dst.get()
    src.close()
    dst.close()
    # every row read the same state and the same token: the same bits of h and c in every layer, whatever tile the row sits in
    for a in (got['h'], got['c']):
        assert np.array_equal(bits(a), bits(np.repeat(a[:, :1], n, 1))), 'rows of one state differ'
    assert got['ctx'][:, 1].tolist() == [int(v) for v in cols]
    res = D.check_cell(params, cfg, tok, h, c, got['h'][:, :1], got['c'][:, :1])
    full = n == O.model_dims(cfg)['V1']
    res['lp'] = D.check_lp(params, got['h'][-1, 0], lp, None if full else cols)
    assert res['lp']['n'] == n and ('sum' in res['lp']) == full
    return res


@pytest.mark.parametrize('shape', D.LP_FULL, ids=lambda s: 'H%d-V%d' % (s[1], s[2]))
def test_full_logit_rows(shape):
    E, H, V1 = shape
    m, cfg, params = seeded_model(E, H, 1, V1 - 1)
    dd = m.debug_dims()
    assert dd['Hp'] == H and dd['V1p'] == D.round_up(V1, 4)
    res = logit_row(m, cfg, params, np.arange(V1))
    assert_ok('H%d-V%d' % (H, V1), res, m)


@pytest.mark.parametrize('V1,staged', D.LP_WIDE)
def test_wide_logit_rows(V1, staged):
    """staged: row_max_lse keeps the row in LDS (V1 <= 32 768, launch_row_kernel); else it reads it from global memory twice"""
    assert staged == (V1 <= D.PICK_LDS_FLOATS)
    m, cfg, params = seeded_model(8, 16, 1, V1 - 1)
    cols = D.checked_columns(V1)
    assert len(cols) == D.MAX_CHECKED
    res = logit_row(m, cfg, params, cols)
    assert_ok('H16-V%d-%s' % (V1, 'staged' if staged else 'unstaged'), res, m)
