"""fsmg_beam_search_constrained / fsmg_dstate_beam_search_constrained / fsmg_maml_beam_search_constrained on the MI355X (DESIGN.md
30) against data.constraints and the fp64 restatement tests/cbeam_ref.py: the NULL constraint, W = 1 against the constrained greedy
draw, a ban through the bias against one through the automaton, exact membership over the table edges, group independence, the
carried state, the hypotheses against fp64 where the gaps are clear, dead ends, the refusals, the MAML variant and the plugin /
train.train surface."""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import cbeam_ref as CB
import constraint_ref as CR
import gen_ref as R
import test_beam as TB
from conftest import small_config
from data.constraints import Constraints, midi_constraints
from gpu_utils import f64_params, new_model

pytestmark = pytest.mark.gpu

TOL = TB.TOL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(input_size, H=16, L=1, max_len=8, E=8):
    return small_config(input_size=input_size, max_len=max_len, embedding_size=E, hidden_size=H, n_layers=L)


def _same(a, b):
    """tokens, scores and log-probs (and constraint states) equal bitwise"""
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    for x, y in zip(a[3:], b[3:]):
        for k in ('state', 'open', 'dead_ends'):
            assert np.array_equal(x[k], y[k]), k


def _search(m, con, G, W, num, **kw):
    return m.beam_search(num, W, n_groups=G, logprobs=True, constraints=con, return_cstate=True, **kw)


# -------------------------------------------------------------------------------- 1: the NULL constraint
def _raw(m, name, head, tail, G, W, num):
    from fsmg.binding import _I32P, _f32p
    toks = np.zeros((G, W, num), np.int32)
    sc = np.zeros((G, W), np.float32)
    lp = np.zeros((G, W, num), np.float32)
    rc = getattr(m._lib, name)(*head, *tail, toks.ctypes.data_as(_I32P), _f32p(sc), _f32p(lp))
    return rc, toks, sc, lp


@pytest.mark.parametrize('input_size', [97, 50000])
def test_null_constraint_is_the_unconstrained_twin_bitwise(input_size):
    from fsmg.binding import FsmgConstraintState
    m = TB._trained(_cfg(input_size), steps=1)
    G, W, num = 3, 4, 5
    primer = np.random.RandomState(2).randint(0, input_size, size=(G, 3)).astype(np.int32)
    support = np.random.RandomState(4).randint(0, input_size, size=(2, 8)).astype(np.int32)
    sp, slen = C.c_void_p(support.ctypes.data), np.array([5, 8], np.int32)
    st_in, st_out = np.full(G, 7, np.int32), np.full(G * W, 7, np.int32)      # with a NULL constraint neither struct is touched
    cin = FsmgConstraintState(state=st_in.ctypes.data, open=None, dead_ends=None)
    cout = FsmgConstraintState(state=st_out.ctypes.data, open=None, dead_ends=None)
    con_args = (None, C.byref(cin), C.byref(cout))
    for pr in (None, primer):
        P, dev, pp, _keep = m._primer(pr, G, ('n_groups', 'group'))
        b = m.beam_config(G, W, num, P, dev)
        want = _raw(m, 'fsmg_beam_search', (m._h, C.byref(b)), (pp,), G, W, num)
        got = _raw(m, 'fsmg_beam_search_constrained', (m._h, C.byref(b)) + con_args, (pp,), G, W, num)
        assert want[0] == 0 and got[0] == 0
        _same(got[1:], want[1:])
        if input_size != 97:
            continue
        for sl in (None, C.c_void_p(slen.ctypes.data)):
            if sl is None:
                want = _raw(m, 'fsmg_maml_beam_search', (m._h, C.byref(b), sp, 2, 1, 0.1, 0), (pp,), G, W, num)
            else:
                want = _raw(m, 'fsmg_maml_beam_search_masked', (m._h, C.byref(b), sp, sl, 2, 1, 0.1, 0), (pp,), G, W, num)
            got = _raw(m, 'fsmg_maml_beam_search_constrained', (m._h, C.byref(b)) + con_args + (sp, sl, 2, 1, 0.1, 0), (pp,), G, W, num)
            assert want[0] == 0 and got[0] == 0
            _same(got[1:], want[1:])
    out = []
    for name, extra in (('fsmg_dstate_beam_search', ()), ('fsmg_dstate_beam_search_constrained', con_args)):
        s = m.new_state(G, history=32)
        m.feed(s, primer)
        b = m.beam_config(G, W, num)
        out.append(_raw(m, name, (m._h, s._st, C.byref(b)) + extra, (), G, W, num))
        s.close()
    assert out[0][0] == 0 and out[1][0] == 0
    _same(out[1][1:], out[0][1:])
    assert np.all(st_in == 7) and np.all(st_out == 7)


# -------------------------------------------------------------------------------- 2: W = 1 is the constrained greedy draw
@pytest.mark.parametrize('input_size', [97, 4708, 50000])
def test_width_one_is_generate_constrained_at_temperature_zero(input_size):
    V1 = input_size + 1
    cfg = _cfg(input_size)
    m = TB._trained(cfg, steps=1)
    mixed = CR.mixed_constraint(V1, K=33, seed=3)
    banned = Constraints(V1, bias=np.where(np.isfinite(mixed.bias), 0.0, -np.inf), token_class=mixed.token_class,
                         next_state=mixed.next_state, start_state=mixed.start_state, slot_open=mixed.slot_open,
                         slot_close=mixed.slot_close, n_slots=mixed.n_slots)
    G, num = 5, 10
    for con in (banned, mixed):
        for primer in (None, CR.allowed_primer(con, G, 3, seed=1)):
            toks, scores, lps, cs = _search(m, con, G, 1, num, primer=primer)
            want, wlp, wcs = m.generate(G, num, temperature=0.0, primer=primer, logprobs=True, constraints=con, return_cstate=True)
            assert np.array_equal(toks[:, 0], want)
            for k in ('state', 'open', 'dead_ends'):
                assert np.array_equal(cs[k][:, 0], wcs[k]), k
            assert np.all(cs['dead_ends'] == 0)
            if con is banned:           # a bias of 0 or -inf: the log-probs are the same floats
                assert np.array_equal(_bits(lps[:, 0]), _bits(wlp))
        if con is mixed and input_size != 50000:      # a finite bias: lp = z + bias - lse, against fp64 (teacher-forced)
            params = f64_params(m)
            for g in range(G):
                pre = [input_size] + [int(w) for w in primer[g]]
                lg = R.row_logits(params, cfg, pre + [int(w) for w in toks[g, 0, :-1]])[len(pre) - 1:]
                for t in range(num):
                    v = int(toks[g, 0, t])
                    ref = lg[t, v] + float(con.bias[v]) - R.logsumexp(lg[t])
                    assert abs(float(lps[g, 0, t]) - ref) <= TOL, (g, t, lps[g, 0, t], ref)


# -------------------------------------------------------------------------------- 3: a ban through the bias is one through the automaton
@pytest.mark.parametrize('input_size', [97, 4708, 50000])
def test_a_ban_through_the_bias_is_a_ban_through_the_automaton(input_size):
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    banned = np.random.RandomState(1).rand(V1) < 0.6
    banned[-1] = True
    by_bias = Constraints(V1, bias=np.where(banned, -np.inf, 0.0))
    by_automaton = Constraints(V1, token_class=banned.astype(np.int32), next_state=[[0, -1]])
    primer = np.flatnonzero(~banned)[:3][None].repeat(3, 0)
    for W, pr in ((1, None), (4, primer), (64, None)):
        a = _search(m, by_bias, 3, W, 5, primer=pr)
        b = _search(m, by_automaton, 3, W, 5, primer=pr)
        _same(a[:3], b[:3])
        assert not banned[a[0]].any() and np.all(a[3]['dead_ends'] == 0)
        CB.check_walk(by_bias, *a, primer=pr)


# -------------------------------------------------------------------------------- 4: exact membership over the table edges
def _edge(V1, kind, K, S, Cn):
    if kind == 'midi':
        return midi_constraints(max_silence=2)
    return CR.mixed_constraint(V1, K=K, seed=7, S=S, C=Cn)


EDGES = [(98, 'mixed', 0, 1, 1, 1), (98, 'mixed', 32, 3, 4, 4), (98, 'mixed', 33, 256, 64, 64), (4709, 'mixed', 33, 3, 4, 4),
         (4709, 'midi', 2048, 3, 2, 64), (4709, 'mixed', 32, 1, 1, 1), (50001, 'mixed', 4096, 256, 64, 4), (50001, 'mixed', 33, 3, 4, 64),
         (50001, 'mixed', 0, 1, 1, 1)]


@pytest.mark.parametrize('V1,kind,K,S,Cn,W', EDGES, ids=lambda x: str(x))
def test_every_token_lies_in_omega_and_the_state_is_the_walked_one(V1, kind, K, S, Cn, W):
    con = _edge(V1, kind, K, S, Cn)
    assert (con.n_slots, con.n_states, con.n_classes) == (K, S, Cn)
    m = new_model(_cfg(V1 - 1))
    G, num = 3, 6
    primer = CR.allowed_primer(con, G, 4, seed=3)
    for pr in (None, primer):
        out = _search(m, con, G, W, num, primer=pr)
        CB.check_walk(con, *out, primer=pr)
        assert np.all(out[3]['dead_ends'] == 0)
    # from a given state per group: slots open, a state other than the start state, dead ends counted on
    st = [CR.walk_primer(con, primer[g], *con.initial())[:2] for g in range(G)]
    cs_in = dict(state=np.array([s for s, _ in st], np.int32), open=np.stack([o for _, o in st]), dead_ends=np.arange(G, dtype=np.int32))
    out = _search(m, con, G, W, num, cstate=cs_in)
    CB.check_walk(con, *out, cs_in=cs_in)
    assert np.array_equal(out[3]['dead_ends'], np.arange(G)[:, None].repeat(W, 1))
    # ... and any one of the three arrays alone
    alone = _search(m, con, G, W, num, cstate=dict(state=cs_in['state']))
    CB.check_walk(con, *alone, cs_in=dict(state=cs_in['state']))


@pytest.mark.parametrize('input_size', [97, 50000])
def test_fewer_allowed_columns_than_the_width(input_size):
    """|Omega| = 3 < W = 8: a row offers three candidates, the padding never wins, no excluded column is drawn"""
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    bias = np.full(V1, -np.inf, np.float32)
    bias[[5, 40, 96]] = [0.0, 0.5, -1.0]
    con = Constraints(V1, bias=bias)
    out = _search(m, con, 2, 8, 4)
    CB.check_walk(con, *out)
    assert np.all(np.isin(out[0], (5, 40, 96))) and np.all(out[3]['dead_ends'] == 0)
    # from the second position on the 3 x 3 finite candidates fill the beam: 8 finite, distinct hypotheses
    assert np.all(np.isfinite(out[1]))
    # an allowed column whose z^c is -inf or NaN still ranks above every excluded column
    sb = m.get_param('softmax_b')
    sb[5], sb[40], sb[96] = -np.inf, np.nan, -np.inf
    m.set_param('softmax_b', sb)
    out = _search(m, con, 2, 8, 3)
    assert np.all(np.isin(out[0], (5, 40, 96))) and np.all(out[3]['dead_ends'] == 0)


# -------------------------------------------------------------------------------- 5: groups, determinism, no side effects
def test_group_independence_determinism_and_no_handle_state():
    cfg = _cfg(97, H=32, L=2, max_len=12, E=12)
    m = TB._trained(cfg)
    con = CR.mixed_constraint(98, K=33, seed=2)
    primer = CR.allowed_primer(con, 9, 4, seed=0)
    before = TB._state(m)
    a = _search(m, con, 9, 16, 8, primer=primer)
    b = _search(m, con, 9, 16, 8, primer=primer)
    _same(a, b)
    TB._same_state(before, TB._state(m))
    for g in (0, 4, 8):
        alone = _search(m, con, 1, 16, 8, primer=primer[g:g + 1])
        _same(alone, tuple(x[g:g + 1] for x in a[:3]) + ({k: v[g:g + 1] for k, v in a[3].items()},))
    c = _search(m, con, 3, 16, 8, primer=primer[3:6])
    _same(c, tuple(x[3:6] for x in a[:3]) + ({k: v[3:6] for k, v in a[3].items()},))
    dc = m.new_constraint(con)         # a DeviceConstraint made once gives the same as the host object
    _same(a, _search(m, dc, 9, 16, 8, primer=primer))
    dc.close()


# -------------------------------------------------------------------------------- 6: the carried state
@pytest.mark.parametrize('input_size', [97, 4708])
def test_carried_state_equals_the_call_with_the_primer(input_size):
    V1 = input_size + 1
    m = TB._trained(_cfg(input_size), steps=2)         # (two steps: _state reads the last two losses)
    con = midi_constraints(max_silence=2) if V1 == 4709 else CR.mixed_constraint(V1, K=33, seed=4)
    G, W, num = 4, 8, 6
    primer = CR.allowed_primer(con, G, 3, seed=5)
    whole = _search(m, con, G, W, num, primer=primer)
    st = m.new_state(G, history=32)
    m.feed(st, primer)
    s, o = zip(*[CR.walk_primer(con, primer[g], *con.initial())[:2] for g in range(G)])
    cs = dict(state=np.array(s, np.int32), open=np.stack(o), dead_ends=np.zeros(G, np.int32))
    keep = {k: v.copy() for k, v in cs.items()}
    before, sb, info = TB._state(m), st.get(), st.info()
    got = _search(m, con, G, W, num, state=st, cstate=cs)
    _same(got, whole)
    TB._same_state(before, TB._state(m))
    sa = st.get()
    assert st.info() == info and all(np.array_equal(sb[k], sa[k]) for k in sb)
    assert all(np.array_equal(cs[k], keep[k]) for k in cs)           # cstate_in is only read
    st.close()


# -------------------------------------------------------------------------------- 7: against fp64
@pytest.mark.parametrize('H,L', CB.REF_SHAPES)
def test_against_reference_across_hidden_sizes(H, L):
    cfg = CB.ref_config(H, L)
    params = CB.ref_params(cfg, H)
    m = new_model(small_config(**cfg), params=params)
    p64 = f64_params(m)
    con = CR.mixed_constraint(301, K=33, seed=H)
    num = 4
    clear = total = 0
    for G, W, P in CB.REF_CASES:
        primer = CR.allowed_primer(con, G, P, seed=G * W + P) if P else None
        toks, scores, lps, cs = _search(m, con, G, W, num, primer=primer)
        CB.check_walk(con, toks, scores, lps, cs, primer=primer)
        ref = CB.beam_search(p64, cfg, con, G, W, num, primer=primer)
        c, n = CB.check_against(ref, toks, scores, cs, TOL, num)
        clear, total = clear + c, total + n
    print('H x L %d x %d: %d clear groups of %d' % (H, L, clear, total))
    assert 2 * clear >= total, (clear, total)


# -------------------------------------------------------------------------------- 8: dead ends
@pytest.mark.parametrize('H,L', [(16, 1), (48, 2)])
def test_dead_ends_against_the_reference(H, L):
    cfg = _cfg(97, H=H, L=L)
    m = new_model(cfg, params=CB.ref_params(cfg, 3))
    p64 = f64_params(m)
    G, W, num = 2, 4, 5
    con = CB.dead_end_constraint()
    toks, scores, lps, cs = _search(m, con, G, W, num)
    CB.check_walk(con, toks, scores, lps, cs)
    ref = CB.beam_search(p64, cfg, con, G, W, num)
    assert np.all(ref[3] >= 0.02), ref[3]
    assert CB.check_against(ref, toks, scores, cs, TOL, num) == (G, G)
    for g in range(G):      # three live hypotheses, then the one that met four dead ends, which has the highest score
        assert cs['dead_ends'][g].tolist() == [0, 0, 0, num - 1]
        assert scores[g, 3] > scores[g, 0]
    con = CB.dead_end_constraint(all_dead=True)
    toks, scores, lps, cs = _search(m, con, G, W, num)
    CB.check_walk(con, toks, scores, lps, cs)
    assert np.all(cs['dead_ends'] == num - 1) and np.all(cs['state'] == 1) and np.all(np.isin(toks[:, :, 0], (20, 30)))
    # a dead end through the slots: the tokens drawn there leave the open bits alone
    con = CB.slot_dead_end_constraint()
    toks, scores, lps, cs = _search(m, con, G, W, num)
    CB.check_walk(con, toks, scores, lps, cs)
    assert np.all(cs['open'] == 3) and np.all(cs['dead_ends'] == num - 2)
    # a dead-end row is ranked as fsmg_beam_search ranks it: from a dead-end state every position is the unconstrained search's
    dead_in = dict(state=np.ones(G, np.int32))
    got = _search(m, CB.dead_end_constraint(), G, W, num, cstate=dead_in)
    want = m.beam_search(num, W, n_groups=G, logprobs=True)
    _same(got[:3], want)
    assert np.all(got[3]['dead_ends'] == num) and np.all(got[3]['state'] == 1)


# -------------------------------------------------------------------------------- 9: the refusals
def test_refusals_and_primers():
    import torch
    from fsmg.binding import FsmgError, _I32P, _f32p
    m = new_model(_cfg(20))
    con = Constraints(21, token_class=(np.arange(21) % 2).astype(np.int32), next_state=[[1, -1], [0, 1]], slot_open=np.arange(21) - 1,
                      n_slots=20)
    assert m.beam_search(4, 4, n_groups=3, constraints=con)[0].shape == (3, 4, 4)
    for bad in (dict(state=[0, 2, 0]), dict(state=[-1, 0, 0]), dict(dead_ends=[0, -1, 0]), dict(open=[[0], [1 << 20], [0]])):
        with pytest.raises(FsmgError) as e:
            m.beam_search(4, 4, n_groups=3, constraints=con, cstate=bad)
        assert e.value.code == -1, bad
    # what fsmg_beam_search refuses
    for kw in (dict(beam_width=65), dict(beam_width=0), dict(num=0)):
        with pytest.raises(FsmgError) as e:
            m.beam_search(kw.get('num', 4), kw.get('beam_width', 4), n_groups=3, constraints=con)
        assert e.value.code == -1, kw
    with pytest.raises(FsmgError) as e:
        m.beam_search(4, 4, n_groups=3, constraints=con, primer=np.array([[2, 20]] * 3))
    assert e.value.code == -7
    # null outputs, a foreign and a destroyed constraint: errors, the outputs untouched
    dc = m._constraint(con)
    b = m.beam_config(3, 4, 4)
    toks, sc, lp = np.full((3, 4, 4), -5, np.int32), np.full((3, 4), -5.0, np.float32), np.full((3, 4, 4), -5.0, np.float32)
    tp, scp = toks.ctypes.data_as(_I32P), _f32p(sc)
    fn = m._lib.fsmg_beam_search_constrained
    assert fn(m._h, C.byref(b), dc._con, None, None, None, None, scp, None) == -1
    assert fn(m._h, C.byref(b), dc._con, None, None, None, tp, None, None) == -1
    assert fn(m._h, None, dc._con, None, None, None, tp, scp, None) == -1
    other = new_model(_cfg(20))
    assert other._lib.fsmg_beam_search_constrained(other._h, C.byref(b), dc._con, None, None, None, tp, scp, None) == -1
    gone = m.new_constraint(con)
    handle = gone._con
    gone.close()
    assert fn(m._h, C.byref(b), handle, None, None, None, tp, scp, _f32p(lp)) == -1
    st = m.new_state(3, history=8)
    assert m._lib.fsmg_dstate_beam_search_constrained(m._h, st._st, C.byref(b), handle, None, None, tp, scp, None) == -1
    assert m._lib.fsmg_dstate_beam_search_constrained(m._h, None, C.byref(b), dc._con, None, None, tp, scp, None) == -1
    b2 = m.beam_config(2, 4, 4)
    assert m._lib.fsmg_dstate_beam_search_constrained(m._h, st._st, C.byref(b2), dc._con, None, None, tp, scp, None) == -1
    st.close()
    # a host primer token that is not allowed where it stands: refused before any device work
    for primer in ([[3, 2]], [[2, 4, 2]], [[0, 2]]):       # class 1 in state 0; slot 1 opened twice; an allowed one
        pr = np.array(primer * 3, np.int32)
        P, dev, pp, _keep = m._primer(pr, 3, ('n_groups', 'group'))
        bp = m.beam_config(3, 4, 4, P, dev)
        walked = con.first_violation(pr[0])
        rc = fn(m._h, C.byref(bp), dc._con, None, None, pp, tp, scp, _f32p(lp))
        assert rc == (-1 if walked is not None else 0), (primer, walked)
        if walked is not None:
            assert np.all(toks == -5) and np.all(sc == -5.0) and np.all(lp == -5.0)
    # the same token in a device primer: the primer flag
    dp = torch.tensor([[3, 2]] * 3, dtype=torch.int32, device='cuda')
    with pytest.raises(FsmgError) as e:
        m.beam_search(4, 4, n_groups=3, constraints=con, primer=(dp.data_ptr(), 2))
    assert e.value.code == -7
    good = torch.tensor([[2, 5]] * 3, dtype=torch.int32, device='cuda')
    a = m.beam_search(4, 4, n_groups=3, constraints=con, primer=(good.data_ptr(), 2))
    h = m.beam_search(4, 4, n_groups=3, constraints=con, primer=np.array([[2, 5]] * 3))
    assert np.array_equal(a[0], h[0]) and np.array_equal(_bits(a[1]), _bits(h[1]))
    # the MAML variant refuses a bad host primer before it adapts
    theta = m.get_params()
    with pytest.raises(FsmgError) as e:
        m.maml_beam_search(np.ones((2, 8), np.int32), 4, 1, 0.1, 4, n_groups=3, constraints=con, primer=np.array([[3, 2]] * 3))
    assert e.value.code == -1
    for k, v in m.get_params().items():
        assert np.array_equal(_bits(v), _bits(theta[k]))
    with pytest.raises(ValueError):
        m.beam_search(4, 4, n_groups=3, cstate=dict(state=[0, 0, 0]))
    assert m.beam_search(4, 4, n_groups=3)[0].shape == (3, 4, 4)          # the handle stays usable


# -------------------------------------------------------------------------------- 10: the MAML variant
def test_maml_variant_adapts_searches_and_restores():
    cfg = _cfg(60, H=32, max_len=10, E=10)
    m = TB._trained(cfg)
    con = CR.mixed_constraint(61, K=20, seed=3)
    m.debug_set('keep_adapted', 1)
    theta = m.get_params()
    support = np.random.RandomState(4).randint(0, 60, size=(3, 10)).astype(np.int32)
    primer = CR.allowed_primer(con, 2, 3, seed=2)
    for slen in (None, np.array([10, 4, 7], np.int32)):
        got = m.maml_beam_search(support, 6, 2, 0.1, 8, n_groups=2, primer=primer, logprobs=True, support_len=slen, constraints=con,
                                 return_cstate=True)
        for k, v in m.get_params().items():
            assert np.array_equal(_bits(v), _bits(theta[k])), k
        CB.check_walk(con, *got, primer=primer)
        # the plain call on a handle that holds theta' (kept by the call right before it restored theta)
        fast = {k: m.get_adapted(k) for k in m.param_shapes}
        assert any(not np.array_equal(fast[k], theta[k]) for k in theta)
        m2 = new_model(cfg, params=fast)
        _same(got, _search(m2, con, 2, 8, 6, primer=primer))
        assert not np.array_equal(got[1], _search(m, con, 2, 8, 6, primer=primer)[1])


# -------------------------------------------------------------------------------- 11: the plugin and train.train
def test_plugin_beam_search_under_the_midi_preset(tmp_path):
    from data import midi_loader as M
    from data.midi_loader import MIDILoader
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    V = M.OFF_TIME + M.MAX_SHIFT_STEPS
    loader = MIDILoader(12, persist=False)
    con = loader.constraints(max_silence=3)
    support = np.random.RandomState(5).randint(0, V, size=(3, 12)).astype(np.int32)
    for cls in (LSTMBaseline, MAMLLSTM):
        cfg = dict(small_config(input_size=V, max_len=12, embedding_size=8, hidden_size=16), name=cls.__name__.lower(),
                   checkpt_dir=str(tmp_path / cls.__name__), inner_steps=1, inner_lr=0.1)
        model = cls(cfg)
        model.recover_or_init('')
        toks, scores, cs = model.beam_search(support, 16, 6, n=2, constraints=con, return_cstate=True)
        assert toks.shape == (2, 6, 16) and scores.shape == (2, 6) and np.all(cs['dead_ends'] == 0)
        for row in toks.reshape(-1, 16):
            assert con.first_violation(row) is None
            song = loader.detokenize(row)
            n_off = int(np.sum((row >= M.OFF_NOTE_OFF) & (row < M.OFF_VELOCITY)))
            assert sum(len(notes) for _, notes in song.instruments) == n_off
        free = model.beam_search(support, 16, 6, n=2)
        assert not np.array_equal(toks, free[0])
        if cls is LSTMBaseline:
            want = model.engine.beam_search(16, 6, n_groups=2, constraints=con)
            assert np.array_equal(toks, want[0]) and np.array_equal(_bits(scores), _bits(want[1]))
        with pytest.raises(ValueError):
            model.beam_search(support, 16, 6, n=2, return_cstate=True)


def _midi_tree(root, n_artists, n_songs, max_len, V):
    """a MIDI dataset of pre-tokenised songs: empty .mid files with their token sidecars"""
    rs = np.random.RandomState(0)
    for a in range(n_artists):
        d = root / ('artist_%02d' % a)
        d.mkdir(parents=True)
        for s in range(n_songs):
            mid = d / ('song_%d.mid' % s)
            mid.write_bytes(b'')
            np.save(str(mid) + '.%d.npy' % max_len, rs.randint(0, V, size=max_len).astype(np.int32))


def test_train_entry_with_sample_beam_constraints(tmp_path):
    import test_train_entry as E
    import train.train as T
    from data import midi_loader as M
    V = M.OFF_TIME + M.MAX_SHIFT_STEPS
    con = midi_constraints()
    root = tmp_path / 'midi'
    _midi_tree(root, 20, E.K + E.Q, 16, V)
    from models.lstm_baseline import LSTMBaseline
    dumps, passed = {}, {}
    for mode in ('absent', 'none', 'loader'):
        cfg = dict(E.LOOP, name='lstm_baseline', model_module_name='models.lstm_baseline', model_class_name='LSTMBaseline', seed=1,
                   embedding_size=8, hidden_size=16, n_layers=1, lr=1e-3, max_grad_norm=5, n_decay=1000, sample_beam_width=4)
        if mode != 'absent':
            cfg['sample_beam_constraints'] = mode
        tmp = tmp_path / mode
        tmp.mkdir()
        paths = {}
        docs = {'data': dict(dataset='midi', dataset_path=str(root), splits=['train', 'val', 'test'], max_len=16),
                'task': dict(query_size=E.Q, support_size=E.K, seed=1234), 'model': cfg}
        for name, doc in docs.items():
            paths[name] = str(tmp / (name + '.yaml'))
            with open(paths[name], 'w') as f:
                yaml.safe_dump(doc, f)
        ck = str(tmp / 'ck')
        seen = []
        real = M.MIDILoader.detokenize

        def spy(self, numpy_data):          # the token rows the dump hands to the detokenizer, in order
            seen.append([int(w) for w in numpy_data])
            return real(self, numpy_data)
        real_beam = LSTMBaseline.beam_search
        passed[mode] = []

        def beam_spy(self, *a, **kw):
            passed[mode].append(kw.get('constraints'))
            return real_beam(self, *a, **kw)
        M.MIDILoader.detokenize, LSTMBaseline.beam_search = spy, beam_spy
        try:
            T.main(['--data', paths['data'], '--task', paths['task'], '--model', paths['model'], '--checkpt_dir', ck])
        finally:
            M.MIDILoader.detokenize, LSTMBaseline.beam_search = real, real_beam
        per_sample = E.K + 1 + 4            # support songs, model_sample, four hypotheses
        assert len(seen) == cfg['n_samples'] * per_sample
        beams = [seen[i * per_sample + E.K + 1:(i + 1) * per_sample] for i in range(cfg['n_samples'])]
        dumps[mode] = beams
        for i in range(cfg['n_samples']):
            d = os.path.join(ck, 'samples', 'sample_%d' % i)
            assert len([f for f in os.listdir(d) if f.startswith('model_beam_')]) == 4
            sc = [float(x) for x in open(os.path.join(d, 'beam_scores.txt')).read().split()]
            assert len(sc) == 4 and sc == sorted(sc, reverse=True)
    assert dumps['absent'] == dumps['none']           # without the key: the parent's dump
    for hyps in dumps['loader']:
        for row in hyps:
            assert con.first_violation(row) is None, row
    # the key, and nothing else, hands the loader's constraints to the plugin's beam_search
    assert passed['absent'] == [None] * 2 and passed['none'] == [None] * 2
    assert [(c.n_columns, c.n_slots) for c in passed['loader']] == [(V + 1, 2048)] * 2
