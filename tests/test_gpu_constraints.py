"""fsmg_generate_constrained / fsmg_dstate_generate_constrained / fsmg_maml_generate_constrained on the MI355X
against data.constraints and the fp64 restatement tests/constraint_ref.py: six laws (NULL constraint, bias against automaton,
common prefix, exact membership, row independence, carried state), teacher-forced margins, the dead end, the distribution over
Omega, the refusals, and the plugin surface."""
import ctypes as C

import numpy as np
import pytest

import constraint_ref as CR
import gen_ref as R
import test_generate_filters as TF
from conftest import small_config
from data import midi_loader as M
from data.constraints import Constraints, midi_constraints
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

ALL = dict(top_p=0.8, min_p=0.02, repetition_penalty=1.5, repeat_window=0)
FK = {'top_p': 'top_p', 'min_p': 'min_p', 'repetition_penalty': 'theta', 'repeat_window': 'window'}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cfg(input_size, H=16, L=1, max_len=8, E=8):
    return small_config(input_size=input_size, max_len=max_len, embedding_size=E, hidden_size=H, n_layers=L)


def _same(a, b):
    """tokens and log-probs (and constraint states) equal bitwise"""
    assert np.array_equal(a[0], b[0]), (a[0], b[0])
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    for x, y in zip(a[2:], b[2:]):
        for k in ('state', 'open', 'dead_ends'):
            assert np.array_equal(x[k], y[k]), k


def _walk(con, toks, cs_out, primer=None, cs_in=None):
    """law 4, exactly: every token lies in the Omega that Constraints computes from its prefix (any column at a dead end), and the
    returned state, open bits and dead ends are the walked ones"""
    B = toks.shape[0]
    state, opn, dead = CR.initial_cstate(con, B, cs_in)
    for b in range(B):
        s, o, bad = CR.walk_primer(con, [] if primer is None else primer[b], state[b], opn[b])
        assert bad is None
        n_dead = int(dead[b])
        for t, g in enumerate(toks[b].tolist()):
            assert 0 <= g < con.n_columns
            if con.allowed(s, o).any():
                assert con.token_allowed(s, o, g), ('outside Omega', b, t, g, s)
                s, o = con.advance(s, o, g)
            else:
                n_dead += 1
        assert int(cs_out['state'][b]) == s and int(cs_out['dead_ends'][b]) == n_dead, (b, cs_out['state'][b], s)
        assert np.array_equal(np.asarray(cs_out['open']).reshape(B, -1)[b], o), b


# -------------------------------------------------------------------------------- law 1: the NULL constraint
def _raw(m, name, head, tail, B, num):
    from fsmg.binding import _I32P, _f32p
    toks = np.zeros((B, num), np.int32)
    lp = np.zeros((B, num), np.float32)
    rc = getattr(m._lib, name)(*head, *tail, toks.ctypes.data_as(_I32P), _f32p(lp))
    return rc, toks, lp


@pytest.mark.parametrize('input_size', [97, 50000])
def test_law1_null_constraint_is_the_unconstrained_twin_bitwise(input_size):
    from fsmg.binding import FsmgConstraintState
    cfg = _cfg(input_size)
    m = TF._trained(cfg, steps=1)
    primer = np.random.RandomState(2).randint(0, input_size, size=(5, 3))
    support = np.random.RandomState(4).randint(0, input_size, size=(2, 8)).astype(np.int32)
    sp = C.c_void_p(support.ctypes.data)
    slen = np.array([5, 8], np.int32)
    filters = [None, TF._filters(), TF._filters(top_p=1.0, repetition_penalty=1.0)] + [TF._filters(**fk) for fk in TF.FILTER_CASES.values()]
    st = np.full(5, 7, np.int32)                   # with a NULL constraint the state struct is not touched
    io = FsmgConstraintState(state=st.ctypes.data, open=None, dead_ends=None)
    for T, k, pr in ((1.0, 0, None), (0.7, 5, primer), (0.0, 0, primer)):
        for f in filters:
            fp = None if f is None else C.byref(f)
            g, pp, _keep = m._gen_args(5, 6, T, k, 3, pr)
            want = _raw(m, 'fsmg_generate_filtered', (m._h, C.byref(g), fp), (pp,), 5, 6)
            got = _raw(m, 'fsmg_generate_constrained', (m._h, C.byref(g), fp, None, C.byref(io)), (pp,), 5, 6)
            assert want[0] == 0 and got[0] == 0
            _same(got[1:], want[1:])
            assert np.all(st == 7)
            if input_size != 97:
                continue
            for sl in (None, C.c_void_p(slen.ctypes.data)):
                if sl is None:
                    want = _raw(m, 'fsmg_maml_generate_filtered', (m._h, C.byref(g), fp, sp, 2, 1, 0.1, 0), (pp,), 5, 6)
                else:
                    want = _raw(m, 'fsmg_maml_generate_filtered_masked', (m._h, C.byref(g), fp, sp, sl, 2, 1, 0.1, 0), (pp,), 5, 6)
                got = _raw(m, 'fsmg_maml_generate_constrained', (m._h, C.byref(g), fp, None, None, sp, sl, 2, 1, 0.1, 0), (pp,), 5, 6)
                assert want[0] == 0 and got[0] == 0
                _same(got[1:], want[1:])
        # the decode-state variant: two states fed alike
        for f in (None, TF._filters(**TF.FILTER_CASES['penalty'])):
            fp = None if f is None else C.byref(f)
            out = []
            for name, extra in (('fsmg_dstate_generate', ()), ('fsmg_dstate_generate_constrained', (None, None))):
                s = m.new_state(5, history=32)
                m.feed(s, primer)
                g = m.gen_config(5, 6, T, k, 3)
                out.append(_raw(m, name, (m._h, s._st, C.byref(g), fp) + extra, (), 5, 6))
                s.close()
            assert out[0][0] == 0 and out[1][0] == 0
            _same(out[1][1:], out[0][1:])


# -------------------------------------------------------------------------------- law 2: bias against automaton
@pytest.mark.parametrize('input_size', [97, 4708, 50000])
def test_law2_a_ban_through_the_bias_is_a_ban_through_the_automaton(input_size):
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    banned = np.random.RandomState(1).rand(V1) < 0.6
    banned[-1] = True
    by_bias = Constraints(V1, bias=np.where(banned, -np.inf, 0.0))
    by_automaton = Constraints(V1, token_class=banned.astype(np.int32), next_state=[[0, -1]])
    primer = np.flatnonzero(~banned)[:3][None].repeat(5, 0)
    for T, k, fk, pr in ((1.0, 0, {}, None), (0.8, 7, ALL, primer), (0.0, 0, dict(repetition_penalty=1.3), primer)):
        a = m.generate(5, 8, temperature=T, top_k=k, seed=6, primer=pr, logprobs=True, constraints=by_bias, return_cstate=True, **fk)
        b = m.generate(5, 8, temperature=T, top_k=k, seed=6, primer=pr, logprobs=True, constraints=by_automaton, return_cstate=True, **fk)
        _same(a[:2], b[:2])
        assert not banned[a[0]].any() and np.all(a[2]['dead_ends'] == 0)


# -------------------------------------------------------------------------------- law 3: the common prefix
@pytest.mark.parametrize('input_size', [97, 50000])
def test_law3_common_prefix_with_the_unconstrained_draw(input_size):
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    rs = np.random.RandomState(3)
    for T in (1.0, 0.0):
        free, flp = m.generate(7, 12, temperature=T, seed=5, logprobs=True)
        # ban what the unconstrained rows draw at positions 4 .. 11, and a random tenth of the rest
        banned = rs.rand(V1) < 0.1
        banned[np.unique(free[::2, 4:])] = True
        banned[np.unique(free[:, :4])] = False
        con = Constraints(V1, token_class=banned.astype(np.int32), next_state=[[0, -1]])
        toks, lp = m.generate(7, 12, temperature=T, seed=5, logprobs=True, constraints=con)
        for b in range(7):
            out = np.flatnonzero(banned[free[b]])
            n = out[0] if out.size else 12
            assert n >= 4 and np.array_equal(toks[b, :n], free[b, :n]) and np.array_equal(_bits(lp[b, :n]), _bits(flp[b, :n])), (T, b, n)
            assert not banned[toks[b]].any()
        if T > 0:       # (some row does leave the common prefix)
            assert any(banned[free[b]].any() for b in range(7))


# -------------------------------------------------------------------------------- law 4: exact membership, at the table edges
def _edge_constraint(kind, arg):
    if kind == 'midi':
        return 4709, midi_constraints(max_silence=2, instruments=arg)
    arg = dict(arg)
    V1 = arg.pop('V1', 98)
    return V1, CR.mixed_constraint(V1, seed=7, **arg)


EDGES = [('K', dict(K=0)), ('K', dict(K=1)), ('K', dict(K=31)), ('K', dict(K=32)), ('K', dict(K=33)), ('midi', None), ('midi', {2, 9}),
         ('SC', dict(S=1, C=1, K=5)), ('SC', dict(S=256, C=64, K=40)), ('big', dict(V1=50001, K=33)),
         ('big', dict(V1=50001, K=4096, S=256, C=64))]


@pytest.mark.parametrize('which', EDGES, ids=lambda w: '%s-%s' % (w[0], w[1]))
def test_law4_every_token_lies_in_omega_and_the_state_is_the_walked_one(which):
    V1, con = _edge_constraint(*which)
    assert con.n_slots == (2048 if which[0] == 'midi' else which[1]['K'])
    m = new_model(_cfg(V1 - 1))
    primer = CR.allowed_primer(con, 5, 4, seed=3)
    for T, k, fk, pr, B in ((1.0, 0, {}, None, 7), (1.3, 9, ALL, primer, 5), (0.0, 0, {}, primer, 5), (0.0, 0, dict(repetition_penalty=2.0), None, 1)):
        toks, cs = m.generate(B, 14, temperature=T, top_k=k, seed=8, primer=pr, constraints=con, return_cstate=True, **fk)
        _walk(con, toks, cs, primer=pr)
        assert np.all(cs['dead_ends'] == 0)
    # from a given state: slots open, a state other than the start state, dead ends counted on
    s, o = con.initial()
    for w in primer[0]:
        s, o = con.advance(s, o, w)
    cs_in = dict(state=np.full(5, s, np.int32), open=np.tile(o, (5, 1)), dead_ends=np.arange(5, dtype=np.int32))
    toks, cs = m.generate(5, 9, temperature=1.0, seed=2, constraints=con, cstate=cs_in, return_cstate=True)
    _walk(con, toks, cs, cs_in=cs_in)
    assert cs['dead_ends'].tolist() == list(range(5))


def test_law4_no_allowed_column_above_minus_inf_picks_the_lowest_of_omega():
    """softmax_b = -inf on every allowed column but banned ones finite: the pick never leaves Omega, sampling or greedy"""
    b = np.zeros(12, np.float32)
    allowed = np.zeros(12, bool)
    allowed[[5, 7, 10]] = True
    b[allowed] = -np.inf
    b[3] = np.nan
    m = TF._bias_model(b)
    con = Constraints(12, token_class=(~allowed).astype(np.int32), next_state=[[0, -1]])
    for T, k, fk in ((1.0, 0, {}), (0.0, 0, {}), (0.7, 3, ALL), (1.0, 0, dict(top_p=0.5))):
        toks, cs = m.generate(5, 6, temperature=T, top_k=k, seed=1, constraints=con, return_cstate=True, **fk)
        assert np.all(toks == 5) and np.all(cs['dead_ends'] == 0), (T, k, fk, toks)
    # one allowed column finite: always that one; an allowed NaN column is never drawn while it is there
    b[10] = -3.0
    b[7] = np.nan
    m2 = TF._bias_model(b)
    for T in (1.0, 0.0):
        assert np.all(m2.generate(5, 6, temperature=T, seed=1, constraints=con) == 10)


# -------------------------------------------------------------------------------- law 5: rows, determinism, no side effects
def test_law5_row_independence_determinism_and_no_handle_state():
    cfg = _cfg(97, H=32, L=2, max_len=12, E=12)
    m = TF._trained(cfg)
    con = CR.mixed_constraint(98, K=33, seed=2)
    primer = CR.allowed_primer(con, 40, 4, seed=0)
    before = TF._state(m)
    a = m.generate(7, 14, temperature=1.0, top_k=30, seed=42, primer=primer[:7], logprobs=True, constraints=con, return_cstate=True, **ALL)
    b = m.generate(7, 14, temperature=1.0, top_k=30, seed=42, primer=primer[:7], logprobs=True, constraints=con, return_cstate=True, **ALL)
    _same(a, b)
    TF._same_state(before, TF._state(m))
    c = m.generate(7, 14, temperature=1.0, top_k=30, seed=43, primer=primer[:7], constraints=con, **ALL)
    assert not np.array_equal(a[0], c)
    d = m.generate(40, 14, temperature=1.0, top_k=30, seed=42, primer=primer, logprobs=True, constraints=con, return_cstate=True, **ALL)
    _same(a, (d[0][:7], d[1][:7], {k: v[:7] for k, v in d[2].items()}))
    one = m.generate(1, 14, temperature=1.0, top_k=30, seed=42, primer=primer[:1], logprobs=True, constraints=con, return_cstate=True, **ALL)
    _same(one, (a[0][:1], a[1][:1], {k: v[:1] for k, v in a[2].items()}))
    # a DeviceConstraint made once gives the same as the host object
    dc = m.new_constraint(con)
    e = m.generate(7, 14, temperature=1.0, top_k=30, seed=42, primer=primer[:7], logprobs=True, constraints=dc, return_cstate=True, **ALL)
    _same(a, e)
    dc.close()


# -------------------------------------------------------------------------------- law 6: the carried state
@pytest.mark.parametrize('input_size', [97, 4708])
def test_law6_carried_state_in_pieces_equals_one_call(input_size):
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    con = midi_constraints(max_silence=2) if V1 == 4709 else CR.mixed_constraint(V1, K=33, seed=4)
    primer = CR.allowed_primer(con, 5, 3, seed=5)
    fk = dict(top_p=0.9, repetition_penalty=1.3, repeat_window=6)

    def run(pieces):
        st = m.new_state(5, history=32)
        m.feed(st, primer)             # (a fresh state has the start word pending: the rows have now read [start, primer[:-1]])
        s, o = zip(*[CR.walk_primer(con, primer[b], *con.initial())[:2] for b in range(5)])
        cs = dict(state=np.array(s, np.int32), open=np.stack(o), dead_ends=np.zeros(5, np.int32))
        toks, lps = [], []
        for n in pieces:
            t, lp, cs = m.generate(5, n, temperature=1.1, top_k=40, seed=9, logprobs=True, state=st, constraints=con, cstate=cs,
                                   return_cstate=True, **fk)
            toks.append(t)
            lps.append(lp)
        info = st.info()
        st.close()
        return np.concatenate(toks, 1), np.concatenate(lps, 1), cs, info

    whole = run([10])
    _walk(con, whole[0], whole[2], cs_in=None, primer=primer)
    for pieces in ([4, 6], [1, 3, 2, 1, 3]):
        got = run(pieces)
        _same(got[:3], whole[:3])
        assert got[3] == whole[3]
    # and the one-shot call with the primer is the same draw
    one = m.generate(5, 10, temperature=1.1, top_k=40, seed=9, logprobs=True, primer=primer, constraints=con, return_cstate=True, **fk)
    _same(one, whole[:3])


# -------------------------------------------------------------------------------- margins against fp64
def _margins(m, cfg, con, B, num, T, k, seed, fk, primer=None, params=None, maml=None):
    kw = dict(temperature=T, top_k=k, seed=seed, primer=primer, logprobs=True, constraints=con, return_cstate=True, **fk)
    toks, lps, cs = m.generate(B, num, **kw) if maml is None else m.maml_generate(maml, num, 2, 0.1, n_seq=B, **kw)
    return CR.check_margins(f64_params(m) if params is None else params, cfg, con, toks, lps, T, k, seed, primer=primer, cstate_out=cs,
                            **{FK[a]: v for a, v in fk.items()})


@pytest.mark.parametrize('H,L', [(24, 1), (200, 2), (512, 1), (1024, 2)])
def test_margins_across_hidden_sizes(H, L):
    cfg = small_config(input_size=300, max_len=16, embedding_size=20, hidden_size=H, n_layers=L)
    m = TF._trained(cfg)
    con = CR.mixed_constraint(301, K=33, seed=H)
    near = _margins(m, cfg, con, 5, 10, 1.0, 0, 11, ALL)
    print('near-tie positions skipped: %d' % near)
    assert near <= 3
    _margins(m, cfg, con, 5, 8, 0.7, 20, 12, ALL, primer=CR.allowed_primer(con, 5, 6, seed=1))


@pytest.mark.parametrize('input_size', [4708, 50000])
def test_margins_midi_preset_and_unstaged_row(input_size):
    cfg = _cfg(input_size)
    m = TF._trained(cfg, steps=1)
    con = midi_constraints(max_silence=3) if input_size == 4708 else CR.mixed_constraint(50001, K=33, S=5, C=7, seed=1)
    _margins(m, cfg, con, 5, 6, 1.0, 0, 9, ALL, primer=CR.allowed_primer(con, 5, 4, seed=2))
    _margins(m, cfg, con, 1, 6, 0.5, 40, 9, dict(top_p=0.9))
    _margins(m, cfg, con, 5, 6, 0.0, 0, 9, dict(repetition_penalty=1.5, repeat_window=3))


def test_margins_maml_generate_constrained_adapts_and_restores():
    cfg = _cfg(60, H=32, max_len=10, E=10)
    m = TF._trained(cfg)
    con = CR.mixed_constraint(61, K=20, seed=3)
    theta = m.get_params()
    support = np.random.RandomState(4).randint(0, 60, size=(3, 10)).astype(np.int32)
    fast, _ = O.maml_adapt({k: v.astype(np.float64) for k, v in theta.items()}, support[None], cfg, inner_steps=2, inner_lr=0.1)
    _margins(m, cfg, con, 5, 10, 1.0, 0, 8, ALL, params=fast, maml=support)
    for k, v in m.get_params().items():
        assert np.array_equal(_bits(v), _bits(theta[k])), k
    # with support lengths: the masked adaptation's theta', the same pick
    a, cs = m.maml_generate(support, 8, 2, 0.1, n_seq=5, seed=8, constraints=con, support_len=np.array([10, 4, 7], np.int32),
                            return_cstate=True)
    _walk(con, a, cs)


# -------------------------------------------------------------------------------- the dead end
@pytest.mark.parametrize('input_size', [97, 50000])
def test_dead_end_is_counted_picked_unconstrained_and_leaves_the_state(input_size):
    V1 = input_size + 1
    m = new_model(_cfg(input_size))
    bias = np.full(V1, -np.inf, np.float32)
    bias[[11, 40]] = 0.0
    so = np.full(V1, -1, np.int32)
    so[11], so[40] = 0, 33
    con = Constraints(V1, bias=bias, token_class=np.zeros(V1, np.int32), next_state=[[1], [0]], slot_open=so, n_slots=34)
    fk = dict(top_p=0.95, repetition_penalty=1.2, repeat_window=4)
    sa, sb = m.new_state(5, history=16), m.new_state(5, history=16)
    toks, lps, cs = m.generate(5, 6, temperature=1.0, seed=3, logprobs=True, state=sa, constraints=con, return_cstate=True, **fk)
    assert np.all(np.sort(toks[:, :2], axis=1) == [11, 40])                  # two picks, then nothing is allowed
    assert cs['dead_ends'].tolist() == [4] * 5 and cs['state'].tolist() == [0] * 5       # two advances: state 1, then 0
    assert np.all(cs['open'] == np.array([1, 2], np.uint32))
    # the same two picks, then the unconstrained generator from the same decode state and Philox position
    t2, l2, cs2 = m.generate(5, 2, temperature=1.0, seed=3, logprobs=True, state=sb, constraints=con, return_cstate=True, **fk)
    t4, l4 = m.generate(5, 4, temperature=1.0, seed=3, logprobs=True, state=sb, **fk)
    assert np.array_equal(toks, np.concatenate([t2, t4], 1)) and np.array_equal(_bits(lps), _bits(np.concatenate([l2, l4], 1)))
    assert cs2['dead_ends'].tolist() == [0] * 5
    sa.close()
    sb.close()


# -------------------------------------------------------------------------------- the distribution over Omega
def test_distribution_over_omega():
    """V1 = 12, many rows at one position: the frequencies against softmax(z^c / T) over Omega (four columns: df = 3), with the
    statistic and the bound of test_generate_filters.py's distribution test"""
    LN2 = TF.LN2
    b = np.array([1.0, 0.0, 0.5, -LN2, 2.0, -2 * LN2, 0.3, -2 * LN2, 0.0, 1.5, -1.0, 0.0], np.float32)
    m = TF._bias_model(b)
    omega = [1, 3, 5, 7]
    bias = np.full(12, -np.inf, np.float32)
    bias[omega] = [0.0, 0.0, 0.0, 0.5]
    con = Constraints(12, bias=bias)
    for T, seed in ((1.0, 1), (2.0, 2)):
        toks = m.generate(16384, 4, temperature=T, seed=seed, constraints=con)
        counts = np.bincount(toks.ravel(), minlength=12).astype(np.float64)
        zc = (b[omega].astype(np.float64) + bias[omega]) / T
        p = np.exp(zc - R.logsumexp(zc))
        chi2 = np.sum((counts[omega] - p * toks.size) ** 2 / (p * toks.size))
        print('T %g chi2 %.3f counts %s expected %s' % (T, chi2, counts[omega], p * toks.size))
        assert counts[omega].sum() == toks.size and chi2 < TF.CHI2_DF3, (T, chi2, counts, p * toks.size)


# -------------------------------------------------------------------------------- errors
def _config(V1, **kw):
    from fsmg.binding import FsmgConstraintConfig, FSMG_CONSTRAINT_CONFIG_VERSION
    keep = []
    c = FsmgConstraintConfig(version=FSMG_CONSTRAINT_CONFIG_VERSION, n_columns=V1)
    for k, v in kw.items():
        if k == 'reserved':
            c.reserved[v] = 1
        elif k in ('bias', 'token_class', 'next_state', 'slot_open', 'slot_close'):
            a = np.ascontiguousarray(v, np.float32 if k == 'bias' else np.int32)
            keep.append(a)
            setattr(c, k, a.ctypes.data)
        else:
            setattr(c, k, v)
    return c, keep


def _create(m, V1, **kw):
    c, _keep = _config(V1, **kw)         # (the arrays the config points at stay alive through the call)
    h = C.c_void_p()
    rc = m._lib.fsmg_constraint_create(m._h, C.byref(c), C.byref(h))
    if rc == 0:
        assert m._lib.fsmg_constraint_destroy(m._h, h) == 0
    return rc


def test_create_refusals():
    m = new_model(_cfg(20))
    V1 = 21
    z, mo = np.zeros(V1), np.full(V1, -1)
    good = [dict(), dict(bias=np.full(V1, -np.inf)), dict(token_class=z, next_state=[0], n_states=1, n_classes=1),
            dict(slot_open=np.arange(V1) - 1, n_slots=20), dict(token_class=z, next_state=np.zeros((256, 64)), n_states=256, n_classes=64),
            dict(n_slots=4096)]
    for kw in good:
        assert _create(m, V1, **kw) == 0, kw
    one = np.where(np.arange(V1) == 3, 0, -1)
    bad = [dict(version=2), dict(version=0), dict(reserved=0), dict(reserved=9), dict(n_columns=20), dict(n_columns=22),
           dict(bias=np.where(np.arange(V1) == 2, np.inf, 0)), dict(bias=np.where(np.arange(V1) == 2, np.nan, 0)),
           dict(token_class=z), dict(next_state=[0], n_states=1, n_classes=1), dict(n_states=1, n_classes=1), dict(start_state=1),
           dict(token_class=z, next_state=[0], n_states=0, n_classes=1), dict(token_class=z, next_state=[0], n_states=1, n_classes=0),
           dict(token_class=z, next_state=np.zeros((257, 1)), n_states=257, n_classes=1),
           dict(token_class=z, next_state=np.zeros((1, 65)), n_states=1, n_classes=65),
           dict(token_class=np.where(np.arange(V1) == 20, 2, 0), next_state=[0, 0], n_states=1, n_classes=2),
           dict(token_class=np.where(np.arange(V1) == 0, -1, 0), next_state=[0], n_states=1, n_classes=1),
           dict(token_class=z, next_state=[1], n_states=1, n_classes=1), dict(token_class=z, next_state=[-2], n_states=1, n_classes=1),
           dict(token_class=z, next_state=[0, 0], n_states=2, n_classes=1, start_state=2),
           dict(token_class=z, next_state=[0, 0], n_states=2, n_classes=1, start_state=-1),
           dict(slot_open=one, n_slots=0), dict(slot_close=one + np.where(np.arange(V1) == 3, 5, 0), n_slots=5),
           dict(slot_open=mo - 1, n_slots=4), dict(slot_open=one, slot_close=one, n_slots=1), dict(n_slots=-1), dict(n_slots=4097)]
    for kw in bad:
        assert _create(m, V1, **kw) == -1, kw
    assert m._lib.fsmg_constraint_create(m._h, None, C.byref(C.c_void_p())) == -1
    assert m._lib.fsmg_constraint_create(m._h, C.byref(_config(V1)[0]), None) == -1
    # a foreign or destroyed constraint is an error, not a crash
    dc = m.new_constraint(Constraints(V1))
    other = new_model(_cfg(20))
    out = (C.c_int64 * 4)()
    assert m._lib.fsmg_constraint_info(m._h, dc._con, out) == 0 and list(out) == [21, 1, 1, 0]
    assert other._lib.fsmg_constraint_info(other._h, dc._con, out) == -1
    assert other._lib.fsmg_constraint_destroy(other._h, dc._con) == -1
    handle = dc._con
    dc.close()
    assert m._lib.fsmg_constraint_info(m._h, handle, out) == -1
    g = m.gen_config(2, 3)
    toks = np.full((2, 3), -5, np.int32)
    from fsmg.binding import _I32P
    assert m._lib.fsmg_generate_constrained(m._h, C.byref(g), None, handle, None, None, toks.ctypes.data_as(_I32P), None) == -1
    assert np.all(toks == -5)
    assert m.generate(2, 3, seed=1).shape == (2, 3)          # the handle stays usable


def test_call_refusals_and_primers():
    import torch
    from fsmg.binding import FsmgError
    m = new_model(_cfg(20))
    con = Constraints(21, token_class=(np.arange(21) % 2).astype(np.int32), next_state=[[1, -1], [0, 1]], slot_open=np.arange(21) - 1,
                      n_slots=20)
    ok = m.generate(3, 4, seed=1, constraints=con)
    assert ok.shape == (3, 4)
    for bad in (dict(state=[0, 2, 0]), dict(state=[-1, 0, 0]), dict(dead_ends=[0, -1, 0]), dict(open=[[0], [1 << 20], [0]])):
        with pytest.raises(FsmgError) as e:
            m.generate(3, 4, seed=1, constraints=con, cstate=bad)
        assert e.value.code == -1, bad
    # what the unconstrained twin refuses
    with pytest.raises(FsmgError) as e:
        m.generate(3, 4, seed=1, constraints=con, top_p=1.5)
    assert e.value.code == -1
    with pytest.raises(FsmgError) as e:
        m.generate(3, 4, seed=1, constraints=con, primer=np.array([[2, 20]] * 3))
    assert e.value.code == -7
    # a host primer token that is not allowed where it stands: refused before any device work, the outputs untouched
    from fsmg.binding import _I32P, _f32p
    assert [con.first_violation(p) for p in ([3, 2], [2, 4, 2], [0, 2])] == [0, 2, None]
    for primer in ([[3, 2]], [[2, 4, 2]], [[0, 2]]):       # class 1 in state 0; slot 1 opened twice; an allowed one
        pr = np.array(primer * 3, np.int32)
        g, pp, _keep = m._gen_args(3, 4, 1.0, 0, 1, pr)
        toks, lp = np.full((3, 4), -5, np.int32), np.full((3, 4), -5.0, np.float32)
        dc = m._constraint(con)
        walked = con.first_violation(pr[0])
        rc = m._lib.fsmg_generate_constrained(m._h, C.byref(g), None, dc._con, None, pp, toks.ctypes.data_as(_I32P), _f32p(lp))
        assert rc == (-1 if walked is not None else 0), (primer, walked)
        if walked is not None:
            assert np.all(toks == -5) and np.all(lp == -5.0)
    # the same token in a device primer: the primer flag
    dp = torch.tensor([[3, 2]] * 3, dtype=torch.int32, device='cuda')
    with pytest.raises(FsmgError) as e:
        m.generate(3, 4, seed=1, constraints=con, primer=(dp.data_ptr(), 2))
    assert e.value.code == -7
    good = torch.tensor([[2, 5]] * 3, dtype=torch.int32, device='cuda')
    a = m.generate(3, 4, seed=1, constraints=con, primer=(good.data_ptr(), 2))
    assert np.array_equal(a, m.generate(3, 4, seed=1, constraints=con, primer=np.array([[2, 5]] * 3)))
    # the MAML variant refuses a bad host primer before it adapts
    theta = m.get_params()
    with pytest.raises(FsmgError) as e:
        m.maml_generate(np.ones((2, 8), np.int32), 4, 1, 0.1, n_seq=3, constraints=con, primer=np.array([[3, 2]] * 3))
    assert e.value.code == -1
    for k, v in m.get_params().items():
        assert np.array_equal(_bits(v), _bits(theta[k]))
    with pytest.raises(ValueError):
        m.generate(3, 4, cstate=dict(state=[0, 0, 0]))


# -------------------------------------------------------------------------------- the plugin surface
def test_plugin_generate_under_the_midi_preset(tmp_path):
    from data.midi_loader import MIDILoader
    from data.base_loader import Loader
    from models.lstm_baseline import LSTMBaseline
    from models.maml_lstm import MAMLLSTM
    V = M.OFF_TIME + M.MAX_SHIFT_STEPS
    loader = MIDILoader(12, persist=False)
    con = loader.constraints(max_silence=3)
    assert Loader(12, persist=False).constraints() is None and loader.get_num_tokens() == V
    support = np.random.RandomState(5).randint(0, V, size=(3, 12)).astype(np.int32)
    for cls in (LSTMBaseline, MAMLLSTM):
        cfg = dict(small_config(input_size=V, max_len=12, embedding_size=8, hidden_size=16), name=cls.__name__.lower(),
                   checkpt_dir=str(tmp_path / cls.__name__), inner_steps=1, inner_lr=0.1)
        model = cls(cfg)
        model.recover_or_init('')
        toks, cs = model.generate(support, 16, n=5, temperature=1.2, seed=3, top_p=0.95, constraints=con, return_cstate=True)
        assert toks.shape == (5, 16) and np.all(cs['dead_ends'] == 0)
        for row in toks:
            assert con.first_violation(row) is None
            song = loader.detokenize(row)
            n_off = int(np.sum((row >= M.OFF_NOTE_OFF) & (row < M.OFF_VELOCITY)))
            assert sum(len(notes) for _, notes in song.instruments) == n_off
            run = 0
            for w in row:
                run = run + 1 if w >= M.OFF_TIME else 0
                assert run <= 3
        assert np.array_equal(toks, model.generate(support, 16, n=5, temperature=1.2, seed=3, top_p=0.95, constraints=con))
        assert not np.array_equal(toks, model.generate(support, 16, n=5, temperature=1.2, seed=3, top_p=0.95))
