"""-m gpu: batched passes from a carried LSTM state (include/fsmg.h fsmg_*_state).

Every recurrence family imports a state at least once (CASES: the rows and environment that select it, asserted from fsmg_stats,
backward_ref.expected_dispatch and the handle's import tally).  Bitwise laws L1-L7 first, then three consecutive segments -- the last
one ragged -- against the fp64 restatement of tests/state_ref.py: log-probs element-wise within max(NLL_RTOL |fp64|, 8 e32), the loss
within NLL_RTOL, every gradient tensor's rel_max under max(REL_MAX, 8 e32), the exported h, c under max(HS_RTOL, 8 e32); e32 is the same
restatement in fp32 numpy.  Measured figures: tests/COMPONENTWISE_STATE.md.
"""
import numpy as np
import pytest

import backward_ref as R
import dropout_ref as D
import maml_ref as MA
import state_ref as S
from gpu_utils import new_model, rel_max
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-4                # tests/test_gpu_parity.py: a loss against fp64
REL_MAX = 5e-4                 # tests/test_gpu_dyneval.py: a tensor against fp64
HS_RTOL = 2e-5                 # tests/test_gpu_parity.py: Hs / Cs against fp64
HAND_HF, HAND_HX32, HAND_HX16 = 1, 2, 3     # fsmg_debug_read("state_imports"), csrc/fsmg_kernels.h STATE_HAND_*

# (id, index into maml_ref.MAML_SHAPES, rows, environment, forward family, import kind)
CASES = [
    ('per-step', 0, 3, dict(FSMG_PERSISTENT='0'), ('step', 'patch'), HAND_HF),
    ('two-layers', 1, 5, {}, ('step', 'patch'), HAND_HF),                                  # hidden 32: no persistent kernel takes it
    ('slice', 2, 25, {}, ('xcd',), HAND_HX32),
    ('xcd-fp32', 3, 15, {}, ('xcd',), HAND_HX32),
    ('xcd-bf16', 4, 80, {}, ('xcd',), HAND_HX16),
    ('pair-fp32', 5, 10, {}, ('xcd',), HAND_HX32),
    ('pair-bf16', 5, 35, {}, ('xcd',), HAND_HX16),
    ('column-split', 3, 15, dict(FSMG_XCD='0'), ('chain', 'chain_rt'), HAND_HF),
]
IDS = [c[0] for c in CASES]
SERIAL = dict(FSMG_XCD_OVERLAP='0', FSMG_OVERLAP='0')


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def setup(case, monkeypatch, env=None):
    name, idx, rows, cenv, fam, kind = case
    cfg = MA.config_of(MA.MAML_SHAPES[idx], max_grad_norm=5)
    for k, v in dict(cenv, **(env or {})).items():
        monkeypatch.setenv(k, v)
    return cfg, rows


def model_of(cfg, rows):
    return new_model(cfg, MA.initial_theta(cfg), max_sequences=rows)


def check_family(model, case, cfg, rows, train):
    """the family the case is about ran, and imported a state"""
    name, idx, _, cenv, fam, kind = case
    want = R.expected_dispatch(cfg, rows, dict(cenv))
    assert want['fwd'] in fam, (name, want)
    st = model.stats()
    assert st['timeouts'] == 0
    if want['fwd'] == 'xcd':
        assert st['xcd_launches'] > 0 and st['step_launches'] == 0
        assert bool(model.debug_read('xcd_bx3', 1)[0]) == (kind == HAND_HX16), name
    elif want['fwd'] in ('chain', 'chain_rt'):
        assert st['persistent_launches'] > 0 and st['xcd_launches'] == 0 and st['step_launches'] == 0
    else:
        assert st['step_launches'] > 0 and st['xcd_launches'] == 0 and st['persistent_launches'] == 0
    imports = model.debug_read('state_imports', 4)
    assert imports[kind] > 0 and imports.sum() == imports[kind], (name, imports)


def state_of(m):
    out = {}
    for k in m.param_shapes:
        mm, vv = m.get_opt_state(k)
        out[k] = (m.get_param(k), mm, vv)
    return out


def same_state(a, b, what):
    for k in a:
        for x, y, part in zip(a[k], b[k], ('param', 'adam_m', 'adam_v')):
            assert np.array_equal(bits(x), bits(y)), (what, k, part)


def grads_of(m):
    return {k: m.get_grad(k) for k in m.param_shapes}


def same_dstate(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ('h', 'c')) and np.array_equal(a['ctx'], b['ctx']) and \
        a['n_ctx'] == b['n_ctx'] and a['n_gen'] == b['n_gen']


# ----------------------------------------------------------------------------- L1: a fresh state is the masked pass
@pytest.mark.parametrize('order', ['serial', 'default'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_L1_fresh_state_equals_the_masked_calls(case, order, monkeypatch):
    cfg, rows = setup(case, monkeypatch, SERIAL if order == 'serial' else None)
    T = cfg['max_len']
    seg = S.segments(cfg, rows, 2, 11)
    ln = S.ragged_lengths(np.random.RandomState(5), rows, T)
    ln1 = np.maximum(ln, 1)                        # the masked calls take lengths in [1, T]
    a, b = model_of(cfg, rows), model_of(cfg, rows)
    st = b.new_state(rows, history=8)
    # score
    want = a.score(seg[0], rank=True, entropy=True, argmax=True, lengths=ln1, pass_rows=min(rows, 1024))
    got = b.score_state(st, seg[0], ln1, rank=True, entropy=True, argmax=True)
    for k in ('logprob', 'rank', 'entropy', 'argmax', 'row_nll'):
        assert np.array_equal(np.asarray(got[k]).view(np.uint32), np.asarray(want[k]).view(np.uint32)), k
    # eval
    st.reset()
    nll, nv = b.eval_step_state(st, seg[0], ln1)
    assert np.float32(nll).view(np.uint32) == np.float32(a.eval_step_masked(seg[0].reshape(1, rows, T), ln1.reshape(1, rows))).view(np.uint32)
    assert nv == int(ln1.sum())
    # forward + backward, then the update
    st.reset()
    # (the masked twins as one support row and rows - 1 query rows: the same rows in the same order, one group)
    a.forward_backward_masked(seg[0][:1].reshape(1, 1, T), seg[0][1:].reshape(1, rows - 1, T), ln1[:1], ln1[1:])
    b.forward_backward_state(st, seg[0], ln1)
    ga, gb = grads_of(a), grads_of(b)
    for k in ga:
        assert np.array_equal(bits(ga[k]), bits(gb[k])), k
    la, lb = a.apply_update(1.0), b.apply_update(1.0)
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    same_state(state_of(a), state_of(b), 'forward_backward + apply')
    # the fused step (a second update on both)
    st.reset()
    la = a.train_step_masked(seg[1][:1].reshape(1, 1, T), seg[1][1:].reshape(1, rows - 1, T), ln1[:1], ln1[1:])
    lb = b.train_step_state(st, seg[1], ln1)
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    same_state(state_of(a), state_of(b), 'train_step')
    assert a.step == b.step == 2
    check_family(b, case, cfg, rows, True)


# ----------------------------------------------------------------------------- L2, L3: what the state holds afterwards
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_L2_L3_exported_state_context_and_tokens_behind_the_end(case, monkeypatch):
    cfg, rows = setup(case, monkeypatch)
    T, H, L, V = cfg['max_len'], cfg['hidden_size'], cfg['n_layers'], cfg['input_size']
    seg = S.segments(cfg, rows, 2, 12)
    ln = S.ragged_lengths(np.random.RandomState(6), rows, T)
    m = model_of(cfg, rows)
    st = m.new_state(rows, history=T + 2)
    m.forward_backward_state(st, seg[0])                     # a full segment first: the second one starts from a real state
    m.apply_update(1.0)
    before = st.get()
    theta = state_of(m)
    m.forward_backward_state(st, seg[1], ln)
    g1 = grads_of(m)
    after = st.get()
    Hp = m.debug_dims()['Hp']
    for l in range(L):
        hs = m.debug_read('h%d' % l, (T + 1) * rows * Hp).reshape(T + 1, rows, Hp)[:, :, :H]
        cs = m.debug_read('c%d' % l, (T + 1) * rows * Hp).reshape(T + 1, rows, Hp)[:, :, :H]
        assert np.array_equal(bits(hs[0]), bits(before['h'][l])) and np.array_equal(bits(cs[0]), bits(before['c'][l]))       # the import
        for b in range(rows):
            assert np.array_equal(bits(after['h'][l, b]), bits(hs[ln[b], b])), (l, b)
            assert np.array_equal(bits(after['c'][l, b]), bits(cs[ln[b], b])), (l, b)
    assert ln[1] == 0 and np.array_equal(bits(after['h'][:, 1]), bits(before['h'][:, 1]))       # a len == 0 row keeps its state bits
    # the context rule
    last = np.where(ln > 0, seg[1][np.arange(rows), np.maximum(ln - 1, 0)], seg[0][:, -1])
    y = np.where(np.arange(T)[None, :] < ln[:, None], seg[1], last[:, None])
    want_ctx = np.concatenate([seg[0], y], axis=1)[:, -(T + 2):]
    assert after['n_ctx'] == 2 * T and after['n_gen'] == 0 and np.array_equal(after['ctx'], want_ctx)
    assert np.array_equal(after['ctx'][:, -1], last)
    l1 = m.apply_update(1.0)
    # L3: other tokens behind every row's end -- same loss, gradients, state, context
    m2 = model_of(cfg, rows)
    st2 = m2.new_state(rows, history=T + 2)
    m2.forward_backward_state(st2, seg[0])
    m2.apply_update(1.0)
    same_state(theta, state_of(m2), 'same first step')
    rng = np.random.RandomState(99)
    scr = np.where(np.arange(T)[None, :] < ln[:, None], seg[1], rng.randint(0, V, size=seg[1].shape)).astype(np.int32)
    assert not np.array_equal(scr, seg[1])
    m2.forward_backward_state(st2, scr, ln)
    g2 = grads_of(m2)
    for k in g1:
        assert np.array_equal(bits(g1[k]), bits(g2[k])), k
    assert same_dstate(after, st2.get())
    assert np.float32(l1).view(np.uint32) == np.float32(m2.apply_update(1.0)).view(np.uint32)


# ----------------------------------------------------------------------------- L4, L5: refusals and the read-only calls
def test_L4_refused_calls_and_L5_read_only_calls_touch_nothing(monkeypatch):
    case = CASES[3]
    cfg, rows = setup(case, monkeypatch)
    T, V = cfg['max_len'], cfg['input_size']
    seg = S.segments(cfg, rows, 3, 13)
    m, other = model_of(cfg, rows), model_of(cfg, rows)
    st, foreign = m.new_state(rows, history=4), other.new_state(rows, history=4)
    m.train_step_state(st, seg[0])
    keep_s, keep_p, keep_g, step = st.get(), state_of(m), None, m.step
    bad_tok = seg[1].copy()
    bad_tok[2, 3] = V                                  # the start word is not a song token
    refusals = [
        (dict(tokens=seg[1], lengths=np.full(rows, T + 1, np.int32)), 'INVALID'),
        (dict(tokens=seg[1], lengths=np.full(rows, -1, np.int32)), 'INVALID'),
        (dict(tokens=seg[1], lengths=np.zeros(rows, np.int32)), 'INVALID'),
        (dict(tokens=bad_tok, lengths=None), 'TOKEN_RANGE'),
    ]
    calls = [m.score_state, m.eval_step_state, m.forward_backward_state, m.train_step_state]
    for kw, err in refusals:
        for call in calls:
            with pytest.raises(Exception, match=err):
                call(st, **kw)
    for call in calls:                                 # a state of another handle; a wrong version; reserved words
        with pytest.raises(Exception, match='INVALID'):
            m._ck(getattr(m._lib, 'fsmg_' + call.__name__)(m._h, foreign._st, *raw_args(m, seg[1], call.__name__)))
        for field, value in (('version', 2), ('reserved', 1)):
            with pytest.raises(Exception, match='INVALID'):
                m._ck(getattr(m._lib, 'fsmg_' + call.__name__)(m._h, st._st, *raw_args(m, seg[1], call.__name__, **{field: value})))
    big = m.new_state(1025, history=1)
    with pytest.raises(Exception, match='INVALID'):
        m.score_state(big, np.zeros((1025, T), np.int32))
    assert same_dstate(keep_s, st.get()) and m.step == step
    same_state(keep_p, state_of(m), 'refusals')
    # L5
    m.forward_backward_state(st, seg[1])
    keep_g = grads_of(m)
    m.apply_update(1.0)
    keep_p, step = state_of(m), m.step
    m.score_state(st, seg[2])
    m.eval_step_state(st, seg[2])
    same_state(keep_p, state_of(m), 'read-only')
    assert m.step == step and st.info()['n_ctx'] == 4 * T
    for k, g in grads_of(m).items():
        assert np.array_equal(bits(g), bits(keep_g[k])), k


def raw_args(m, tokens, name, version=1, reserved=0):
    import ctypes as C
    from fsmg.binding import FsmgStateConfig, _F32P, _I32P
    c = FsmgStateConfig(version=version, tokens_on_device=0)
    c.reserved[3] = reserved
    tok = np.ascontiguousarray(tokens, np.int32)
    out = np.empty(tok.shape, np.float32)
    raw_args.keep = (c, tok, out, C.c_float(), C.c_int32())
    tp = C.c_void_p(tok.ctypes.data)
    if name == 'score_state':
        return (C.byref(c), tp, None, out.ctypes.data_as(_F32P), None, None, None, None)
    if name == 'eval_step_state':
        return (C.byref(c), tp, None, C.byref(raw_args.keep[3]), C.byref(raw_args.keep[4]))
    if name == 'forward_backward_state':
        return (C.byref(c), tp, None)
    return (C.byref(c), tp, None, C.byref(raw_args.keep[3]))


# ----------------------------------------------------------------------------- L6: dropout enabled, keeps of one
@pytest.mark.parametrize('case', [CASES[1], CASES[4]], ids=[IDS[1], IDS[4]])
def test_L6_dropout_with_keeps_of_one_is_the_undropped_state_pass(case, monkeypatch):
    cfg, rows = setup(case, monkeypatch)
    seg = S.segments(cfg, rows, 2, 14)
    a, b = model_of(cfg, rows), model_of(cfg, rows)
    b.dropout_enable(keep_input=1.0, keep_output=1.0, seed=5)
    sa, sb = a.new_state(rows, history=4), b.new_state(rows, history=4)
    for s in seg:
        la, lb = a.train_step_state(sa, s), b.train_step_state(sb, s)
        assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    same_state(state_of(a), state_of(b), 'keeps of one')
    assert same_dstate(sa.get(), sb.get())
    assert b.dropout_info()['next_pass'] == 2


# ----------------------------------------------------------------------------- L7: a forced time-out
@pytest.mark.parametrize('case', [CASES[2], CASES[3], CASES[6]], ids=[IDS[2], IDS[3], IDS[6]])
def test_L7_forced_time_out_gives_the_per_step_bits_and_advances_once(case, monkeypatch):
    """chain_spin_limit = 0: the persistent kernels give up, the step is skipped on the device -- the export with it -- and repeated on
    per-step launches from the state the first attempt imported"""
    cfg, rows = setup(case, monkeypatch)
    T = cfg['max_len']
    seg = S.segments(cfg, rows, 2, 15)
    ln = S.ragged_lengths(np.random.RandomState(8), rows, T)
    a = model_of(cfg, rows)
    monkeypatch.setenv('FSMG_PERSISTENT', '0')
    b = model_of(cfg, rows)
    sa, sb = a.new_state(rows, history=4), b.new_state(rows, history=4)
    a.debug_set('chain_spin_limit', 0)
    for i, (tok, l) in enumerate(((seg[0], None), (seg[1], ln))):
        la, lb = a.train_step_state(sa, tok, l), b.train_step_state(sb, tok, l)
        assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32), i
        assert same_dstate(sa.get(), sb.get()), i
        same_state(state_of(a), state_of(b), 'segment %d' % i)
    assert a.stats()['timeouts'] == 1 and a.step == 2 and sa.info()['n_ctx'] == 2 * T
    # a forward-only state pass: the same recovery (a fresh handle, so that the persistent kernels are in force again)
    c = model_of(cfg, rows)
    monkeypatch.delenv('FSMG_PERSISTENT')
    d = model_of(cfg, rows)
    sc, sd = c.new_state(rows, history=4), d.new_state(rows, history=4)
    d.debug_set('chain_spin_limit', 0)
    want, got = c.score_state(sc, seg[0]), d.score_state(sd, seg[0])
    assert np.array_equal(bits(want['logprob']), bits(got['logprob'])) and same_dstate(sc.get(), sd.get())
    assert d.stats()['timeouts'] == 1 and sd.info()['n_ctx'] == T


# ----------------------------------------------------------------------------- against fp64
_REF = {}


def reference(case):
    """three consecutive segments, the last one ragged, at constant parameters: the fp64 restatement and its fp32 twin, computed once"""
    name, idx, rows = case[0], case[1], case[2]
    if name not in _REF:
        cfg = MA.config_of(MA.MAML_SHAPES[idx], max_grad_norm=5, lr=0.0)
        T = cfg['max_len']
        seg = S.segments(cfg, rows, 3, 21)
        lens = [None, None, S.ragged_lengths(np.random.RandomState(7), rows, T)]
        theta = MA.initial_theta(cfg)
        out = {}
        for dt in (np.float64, np.float32):
            st, res = S.fresh_state(cfg, rows, dt), []
            for tok, ln in zip(seg, lens):
                r, st = S.segment(theta, st, tok, ln, cfg, dtype=dt)
                res.append((r, st))
            out[dt] = res
        _REF[name] = (cfg, seg, lens, theta, out)
    return _REF[name]


def bound(rtol, ref, e32):
    return np.maximum(rtol * np.abs(ref), 8 * e32)


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_three_segments_against_fp64(case, monkeypatch):
    name, idx, rows, cenv, fam, kind = case
    for k, v in cenv.items():
        monkeypatch.setenv(k, v)
    cfg, seg, lens, theta, ref = reference(case)
    T = cfg['max_len']
    m = new_model(cfg, theta, max_sequences=rows)
    s_train, s_score, s_feed = (m.new_state(rows, history=4) for _ in range(3))
    lp_all = []
    for i, (tok, ln) in enumerate(zip(seg, lens)):
        r64, st64 = ref[np.float64][i]
        r32, st32 = ref[np.float32][i]
        sc = m.score_state(s_score, tok, ln)
        lp_all.append(sc['logprob'])
        e32 = np.abs(r32['logprob'].astype(np.float64) - r64['logprob'])
        err = np.abs(sc['logprob'].astype(np.float64) - r64['logprob'])
        print('STATE|%s|seg %d|logprob|e32 %.3g|device %.3g' % (name, i, e32.max(), err.max()))
        assert np.all(err <= bound(NLL_RTOL, r64['logprob'], e32.max()))
        m.forward_backward_state(s_train, tok, ln)
        grads = {k: m.get_grad(k) for k in m.param_shapes}
        loss = m.apply_update(1.0)                    # lr = 0: the parameters stay
        e32 = abs(float(r32['loss']) - float(r64['loss']))
        print('STATE|%s|seg %d|loss|e32 %.3g|device %.3g' % (name, i, e32 / abs(r64['loss']), abs(loss - r64['loss']) / abs(r64['loss'])))
        assert abs(loss - r64['loss']) <= NLL_RTOL * abs(r64['loss'])
        for k, g in grads.items():
            e32 = rel_max(r32['grads'][k], r64['grads'][k])
            dev = rel_max(g, r64['grads'][k])
            print('STATE|%s|seg %d|%s|e32 %.3g|device %.3g' % (name, i, k, e32, dev))
            assert dev <= max(REL_MAX, 8 * e32), (i, k)
        got = s_train.get()
        for part in ('h', 'c'):
            e32 = rel_max(st32[part], st64[part])
            dev = rel_max(got[part], st64[part])
            print('STATE|%s|seg %d|state %s|e32 %.3g|device %.3g' % (name, i, part, e32, dev))
            assert dev <= max(HS_RTOL, 8 * e32), (i, part)
        assert np.array_equal(got['ctx'], st64['ctx'][:, -4:]) and got['n_ctx'] == (i + 1) * T
        assert same_dstate(got, s_score.get())                      # score and train export the same bits
    # fsmg_dstate_feed of the first two segments' tokens, through the same fp64 values
    fed = m.feed(s_feed, np.concatenate(seg[:2], axis=1), logprobs=True)
    for i in range(2):
        r64, r32 = ref[np.float64][i][0], ref[np.float32][i][0]
        e32 = np.abs(r32['logprob'].astype(np.float64) - r64['logprob']).max()
        err = np.abs(fed[:, i * T:(i + 1) * T].astype(np.float64) - r64['logprob'])
        print('STATE|%s|seg %d|feed logprob|e32 %.3g|device %.3g' % (name, i, e32, err.max()))
        assert np.all(err <= bound(NLL_RTOL, r64['logprob'], e32))
    check_family(m, case, cfg, rows, True)
    assert np.all(m.get_param('softmax_w') == np.float32(theta['softmax_w']))


@pytest.mark.parametrize('case', [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_dropped_state_pass_against_the_numpy_masks(case, monkeypatch):
    name, idx, rows, cenv, fam, kind = case
    for k, v in cenv.items():
        monkeypatch.setenv(k, v)
    cfg, seg, lens, theta, ref = reference(case)
    drop = dict(keep_input=0.8, keep_output=0.5, variational=False, seed=0x0123456789ABCDEF)
    m = new_model(cfg, theta, max_sequences=rows)
    st = m.new_state(rows, history=4)
    m.forward_backward_state(st, seg[0])
    m.apply_update(1.0)
    m.dropout_enable(**drop)
    m.dropout_set_pass(7)
    m.forward_backward_state(st, seg[2], lens[2])
    grads = {k: m.get_grad(k) for k in m.param_shapes}
    loss = m.apply_update(1.0)
    assert m.dropout_info()['last_pass'] == 7
    out = {}
    for dt in (np.float64, np.float32):
        s0 = ref[dt][0][1]                            # the state after segment 0 (recurrent sites are never dropped: the same with dropout on)
        out[dt], _ = S.segment(theta, s0, seg[2], lens[2], cfg, dtype=dt, f=D.factors(cfg, drop, 7, rows, dt))
    assert abs(loss - out[np.float64]['loss']) <= NLL_RTOL * abs(out[np.float64]['loss'])
    for k, g in grads.items():
        e32 = rel_max(out[np.float32]['grads'][k], out[np.float64]['grads'][k])
        dev = rel_max(g, out[np.float64]['grads'][k])
        print('STATE|%s|dropped|%s|e32 %.3g|device %.3g' % (name, k, e32, dev))
        assert dev <= max(REL_MAX, 8 * e32), k


# ----------------------------------------------------------------------------- the plugin, on the golden lyrics
PLUGIN = dict(name='lstm_tbptt', model_module_name='models.tbptt_lstm', model_class_name='TBPTTLSTM', segment_len=12, mask_padding=True,
              n_train=3, print_every_n=3, val_every_n=3.0, n_val=2, n_test=2, n_samples=1, batch_size=2, n_decay=10000, lr=5e-3,
              max_grad_norm=5, embedding_size=24, hidden_size=40, n_layers=1)


def _golden(tmp_path, golden_dir):
    import train.train as T
    from data.episode import load_sampler_from_config
    from test_train_entry import _write_configs
    p = _write_configs(tmp_path, golden_dir, dict(PLUGIN))
    argv = ['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', str(tmp_path / 'ck')]
    config = T.load_config(T.build_parser().parse_args(argv))
    config['split'] = 'train'
    sampler = load_sampler_from_config(config)
    config['input_size'] = sampler.get_num_unique_words()
    return T, argv, config, sampler


def test_plugin_eval_is_the_full_length_nll_and_updates_follow_the_restatement(tmp_path, golden_dir):
    """songs of 32 tokens on a handle of max_len 12: three segments, the last one ragged.  eval = the fp64 NLL of the full-length songs;
    one train(episode) = three updates, each from the state the one before left, against state_ref + the oracle's Adam"""
    T, argv, config, sampler = _golden(tmp_path, golden_dir)
    ep = sampler.get_episode()
    model = T.load_model_from_config(dict(config))
    model.recover_or_init('')
    assert model.n_segments == 3 and model.engine.max_len == 12
    theta = model.engine.get_params()
    V, L32 = config['input_size'], config['max_len']
    qry = ep.query.reshape(-1, L32)
    qlen = ep.query_len.reshape(-1)
    long_cfg = dict(config, max_len=L32)
    X, Y, mask = S.device_xy(qry, qlen, np.full(len(qry), V), V)
    z = S.fresh_state(long_cfg, len(qry))
    want = float(S.run({k: np.asarray(v, np.float64) for k, v in theta.items()}, z['h'], z['c'], X, Y, mask / (qlen.sum() + 1e-12), long_cfg,
                       want_grads=False)['loss'])
    got = model.eval(ep)
    print('STATE|plugin|eval|fp64 %.7f|device %.7f' % (want, got))
    assert abs(got - want) <= NLL_RTOL * abs(want)
    # one train call: the segments in order, an update behind each
    from models.tbptt_lstm import segment_plan, segment_tokens
    songs = np.concatenate([ep.support.reshape(-1, L32), ep.query.reshape(-1, L32)])
    lengths = np.concatenate([ep.support_len.reshape(-1), ep.query_len.reshape(-1)])
    seg_cfg = dict(config, max_len=12)
    out = {}
    for dt in (np.float64, np.float32):
        params = {k: np.asarray(v, dt) for k, v in theta.items()}
        opt, st, num = O.new_opt_state(params), S.fresh_state(seg_cfg, len(songs), dt), 0.0
        for s0, ln in segment_plan(L32, lengths, 12):
            r, st = S.segment(params, st, segment_tokens(songs, s0, 12), ln, seg_cfg, dtype=dt)
            O.apply_update(params, r['grads'], r['aux'], opt, seg_cfg)
            num += float(r['loss']) * int(ln.sum())
        out[dt] = (num / lengths.sum(), params)
    loss = model.train(ep)
    print('STATE|plugin|train loss|fp64 %.7f|device %.7f' % (out[np.float64][0], loss))
    assert abs(loss - out[np.float64][0]) <= NLL_RTOL * abs(out[np.float64][0])
    assert model.global_step() == 3
    after = model.engine.get_params()
    for k in after:
        e32 = rel_max(out[np.float32][1][k], out[np.float64][1][k])
        dev = rel_max(after[k], out[np.float64][1][k])
        print('STATE|plugin|%s after 3 updates|e32 %.3g|device %.3g' % (k, e32, dev))
        assert dev <= max(REL_MAX, 8 * e32), k


def test_plugin_through_train_main(tmp_path, golden_dir, capsys):
    T, argv, config, sampler = _golden(tmp_path, golden_dir)
    T.main(argv)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('Iter: ') or 'Avg NLL' in l]
    assert lines[0].startswith('Iter: 0, val-nll: 5.7')          # ~ln(301) for untrained weights, over segments
    assert any(l.startswith('Iter: 3, loss: ') for l in lines) and any(l.startswith('Test Avg NLL') for l in lines)
    first = float(lines[0].split('val-nll: ')[1])
    last = float([l for l in lines if 'val-nll' in l][-1].split('val-nll: ')[1])
    assert last < first                                            # nine updates (three episodes of three segments)


# ----------------------------------------------------------------------------- device-resident tokens
def test_device_tokens_give_the_host_bits_and_a_bad_one_leaves_the_state_untouched(monkeypatch):
    import torch
    case = CASES[3]
    cfg, rows = setup(case, monkeypatch)
    T, V = cfg['max_len'], cfg['input_size']
    seg = S.segments(cfg, rows, 2, 16)
    ln = S.ragged_lengths(np.random.RandomState(9), rows, T)
    a, b = model_of(cfg, rows), model_of(cfg, rows)
    sa, sb = a.new_state(rows, history=5), b.new_state(rows, history=5)
    dev = [torch.from_numpy(s).cuda() for s in seg]
    torch.cuda.synchronize()
    la, lb = a.train_step_state(sa, seg[0]), b.train_step_state(sb, dev[0].data_ptr())
    assert np.float32(la).view(np.uint32) == np.float32(lb).view(np.uint32)
    want, got = a.score_state(sa, seg[1], ln), b.score_state(sb, dev[1].data_ptr(), ln)
    assert np.array_equal(bits(want['logprob']), bits(got['logprob'])) and same_dstate(sa.get(), sb.get())
    same_state(state_of(a), state_of(b), 'device tokens')
    # an id outside [0, input_size) on the device: found by the pass, which then exports nothing
    bad = seg[0].copy()
    bad[1, 2] = V + 3
    d_bad = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    keep_s, keep_p, step = sb.get(), state_of(b), b.step
    for call in (b.score_state, b.eval_step_state, b.train_step_state):
        with pytest.raises(Exception, match='TOKEN_RANGE'):
            call(sb, d_bad.data_ptr())
    b.forward_backward_state(sb, d_bad.data_ptr())
    with pytest.raises(Exception, match='TOKEN_RANGE'):
        b.apply_update(1.0)
    assert same_dstate(keep_s, sb.get()) and b.step == step
    same_state(keep_p, state_of(b), 'skipped steps')
    lb2, la2 = b.train_step_state(sb, dev[0].data_ptr()), a.train_step_state(sa, seg[0])      # and the handle goes on
    assert np.float32(la2).view(np.uint32) == np.float32(lb2).view(np.uint32) and same_dstate(sa.get(), sb.get())
