"""Decode states (include/fsmg.h fsmg_dstate_*) on the MI355X: the contract E1-E8 bitwise against the one-shot entry points, the
fp64 restatement (tests/dstate_ref.py) and the oracle within the project's bounds, both instantiations of the feed kernel, gather,
get / set, every error, and the plugin / train.train surface."""
import ctypes as C
import os

import numpy as np
import pytest

import dstate_ref as D
import gen_ref as R
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

_I32P = C.POINTER(C.c_int32)
_MODELS = {}


def _trained(steps=3, seed=7, **cfg_over):
    """one trained model per configuration for the whole module (no test changes a model's parameters)"""
    key = tuple(sorted(cfg_over.items())) + (steps,)
    if key not in _MODELS:
        cfg = small_config(**cfg_over)
        m = new_model(cfg)
        for sup, qry in O.synthetic_episodes(steps, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=seed):
            m.train_step(sup, qry)
        _MODELS[key] = (m, cfg)
    return _MODELS[key]


SMALL = dict(input_size=97, max_len=12, embedding_size=12, hidden_size=24)                  # Hp = 32, V1 = 98
TWO_LAYER = dict(input_size=97, max_len=12, embedding_size=12, hidden_size=200, n_layers=2)  # Hp = 256

# generate's keywords: T = 1 with top_k 5; greedy; all three filters with the window as long as the history
PLAIN = dict(temperature=1.0, top_k=5)
GREEDY = dict(temperature=0.0)
FILTERED = dict(temperature=0.9, top_p=0.9, min_p=0.02, repetition_penalty=1.3, repeat_window=5)
SETTINGS = [PLAIN, GREEDY, FILTERED]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return all(np.array_equal(x, y) if x.dtype.kind == 'i' else np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def same_state(a, b):
    ga, gb = a.get(), b.get()
    return (same((ga['h'], ga['c'], ga['ctx']), (gb['h'], gb['c'], gb['ctx'])) and
            (ga['n_ctx'], ga['n_gen']) == (gb['n_ctx'], gb['n_gen']))


def _primer(rows, n, seed=0, vocab=97):
    return np.random.RandomState(seed).randint(0, vocab, size=(rows, n)).astype(np.int32)


@pytest.mark.parametrize('kw', SETTINGS, ids=['plain', 'greedy', 'filtered'])
@pytest.mark.parametrize('shape', [SMALL, TWO_LAYER], ids=['h24', 'h200x2'])
def test_e1_feed_primer_then_generate_is_the_one_shot_call(shape, kw):
    m, cfg = _trained(**shape)
    primer = _primer(3, 4)
    want = m.generate(3, 7, seed=21, primer=primer, logprobs=True, **kw)
    st = m.new_state(3, history=5)                     # shorter than primer + num: only the window has to fit
    assert m.feed(st, primer) is None
    got = m.generate(3, 7, seed=21, logprobs=True, state=st, **kw)
    assert same(got, want)
    assert st.info() == dict(rows=3, history=5, n_ctx=11, n_gen=7)
    st.close()


@pytest.mark.parametrize('kw', SETTINGS, ids=['plain', 'greedy', 'filtered'])
@pytest.mark.parametrize('shape', [SMALL, TWO_LAYER], ids=['h24', 'h200x2'])
def test_e2_chunks_give_the_whole(shape, kw):
    m, cfg = _trained(**shape)
    whole, parts = m.new_state(3, history=5), m.new_state(3, history=5)
    for st in (whole, parts):
        m.feed(st, _primer(3, 1))                      # n_ctx = 1 < the window at the start; it then crosses the call boundary
    want = m.generate(3, 7, seed=4, logprobs=True, state=whole, **kw)
    a = m.generate(3, 3, seed=4, logprobs=True, state=parts, **kw)
    b = m.generate(3, 4, seed=4, logprobs=True, state=parts, **kw)
    assert same((np.concatenate([a[0], b[0]], 1), np.concatenate([a[1], b[1]], 1)), want)
    assert same_state(whole, parts)
    x = _primer(3, 11, seed=2, vocab=98)               # the start word (97) may be fed
    x[1, 4] = 97
    lp = m.feed(whole, x, logprobs=True)
    lp2 = np.concatenate([m.feed(parts, x[:, :5], logprobs=True), m.feed(parts, x[:, 5:], logprobs=True)], 1)
    assert same((lp,), (lp2,)) and same_state(whole, parts)
    assert whole.get()['ctx'].tolist() == x[:, -5:].tolist()
    # without log-probs (the cells-only path) the state is the same
    quiet = m.new_state(3, history=5)
    m.feed(quiet, _primer(3, 1))
    m.generate(3, 7, seed=4, state=quiet, **kw)
    assert m.feed(quiet, x) is None and same_state(whole, quiet)
    for st in (whole, parts, quiet):
        st.close()


def test_whole_context_window_needs_room_in_the_history():
    from fsmg.binding import FsmgError
    m, cfg = _trained(**SMALL)
    pen = dict(temperature=0.9, repetition_penalty=1.3, repeat_window=0)
    primer = _primer(2, 3)
    want = m.generate(2, 6, seed=8, primer=primer, logprobs=True, **pen)
    fits = m.new_state(2, history=9)                   # n_ctx + num = 3 + 6
    m.feed(fits, primer)
    assert same(m.generate(2, 6, seed=8, logprobs=True, state=fits, **pen), want)
    short = m.new_state(2, history=8)                  # one token too small
    m.feed(short, primer)
    before = short.get()
    with pytest.raises(FsmgError) as e:
        m.generate(2, 6, seed=8, state=short, **pen)
    assert e.value.code == -1
    with pytest.raises(FsmgError) as e:
        m.generate(2, 2, seed=8, state=short, temperature=0.9, repetition_penalty=1.3, repeat_window=9)      # window > history
    assert e.value.code == -1
    after = short.get()
    assert same((before['h'], before['c'], before['ctx']), (after['h'], after['c'], after['ctx'])) and after['n_ctx'] == 3
    m.generate(2, 6, seed=8, state=short, temperature=0.9, repeat_window=0)     # no penalty: no rule
    fits.close()
    short.close()


@pytest.mark.parametrize('R_', [1, 65])
def test_e3_feed_scores_generate_and_e4_rows_are_their_own(R_):
    # 65 rows cross k_gen_cell's 64-row block; row 64 of the 65-row state against the same row alone
    m, cfg = _trained(**SMALL)
    primer = _primer(65, 3, seed=5)[65 - R_:]
    st = m.new_state(R_, history=32)
    m.feed(st, primer)
    toks, lps = m.generate(R_, 9, temperature=1.0, seed=6, logprobs=True, state=st)
    again = m.new_state(R_, history=32)
    m.feed(again, primer)
    assert same((m.feed(again, toks, logprobs=True),), (lps,))          # E3
    ga, gb = st.get(), again.get()                      # the same state but for n_gen: 9 generated against 9 given
    assert same((ga['h'], ga['c'], ga['ctx']), (gb['h'], gb['c'], gb['ctx']))
    assert (ga['n_ctx'], ga['n_gen'], gb['n_ctx'], gb['n_gen']) == (12, 9, 12, 0)
    # E4 (the Philox counter holds the row index, so the draw is compared greedy; the fed log-probs at any temperature)
    st.reset()
    m.feed(st, primer)
    g_t, g_l = m.generate(R_, 9, temperature=0.0, logprobs=True, state=st)
    alone = m.new_state(1, history=32)
    m.feed(alone, primer[-1:])
    a_t, a_l = m.generate(1, 9, temperature=0.0, logprobs=True, state=alone)
    assert same((a_t[0], a_l[0]), (g_t[-1], g_l[-1]))
    alone.reset()
    m.feed(alone, primer[-1:])
    assert same((m.feed(alone, toks[-1:], logprobs=True)[0],), (lps[-1],))
    for s in (st, again, alone):
        s.close()


def test_gather():
    m, cfg = _trained(**SMALL)
    primer = _primer(3, 4, seed=9)
    src, dst = m.new_state(3, history=16), m.new_state(4, history=16)
    m.feed(src, primer)
    before = src.get()
    rows = [0, 0, 2, 0]
    dst.gather(src, rows)
    assert dst.info() == dict(rows=4, history=16, n_ctx=4, n_gen=0)
    assert dst.get()['ctx'].tolist() == primer[rows].tolist()
    g = m.generate(4, 8, temperature=0.0, state=dst)
    assert np.array_equal(g[0], g[1]) and np.array_equal(g[0], g[3])
    dst.gather(src, rows)
    got = m.generate(4, 8, temperature=1.0, seed=12, logprobs=True, state=dst)
    assert same(got, m.generate(4, 8, temperature=1.0, seed=12, logprobs=True, primer=primer[rows]))
    after = src.get()
    assert same((before['h'], before['c'], before['ctx']), (after['h'], after['c'], after['ctx']))
    assert src.info()['n_ctx'] == 4 and src.info()['n_gen'] == 0
    src.close()
    dst.close()


@pytest.mark.parametrize('shape', [SMALL, TWO_LAYER], ids=['h24', 'h200x2'])
def test_e5_get_set_round_trip_and_state_against_the_oracle(shape):
    m, cfg = _trained(**shape)
    T, H, L = cfg['max_len'], cfg['hidden_size'], cfg['n_layers']
    songs = _primer(5, T, seed=3)
    st = m.new_state(5, history=7)
    m.feed(st, songs)
    got = st.get()
    assert got['h'].shape == (L, 5, H) and got['c'].shape == (L, 5, H) and got['ctx'].shape == (5, 7)     # H, not the padded width
    assert got['ctx'].tolist() == songs[:, -7:].tolist() and (got['n_ctx'], got['n_gen']) == (T, 0)
    # feed read [start, x_0 .. x_{T-2}]: the oracle's inputs of an eval row, so h and c are its final states (the state bound)
    X, Y = O.eval_xy(songs[None], cfg['input_size'])
    _, cache = O.forward(f64_params(m), X, Y, cfg)
    for l in range(L):
        for name, ref in (('h', cache['layers'][l]['hs'][T]), ('c', cache['layers'][l]['cs'][T])):
            err = np.abs(got[name][l] - ref).max() / np.abs(ref).max()
            print('layer', l, name, 'rel err', err)
            assert err <= 2e-5, (l, name, err)
    # into a fresh state of the same shape, then any call: the same bits; and the same calls again give the same bits
    copy = m.new_state(5, history=7)
    copy.set(got['h'], got['c'], got['ctx'], got['n_ctx'], got['n_gen'])
    assert same_state(st, copy)
    kw = dict(temperature=0.9, top_k=9, top_p=0.95, repetition_penalty=1.2, repeat_window=7, seed=3, logprobs=True)
    a, b = m.generate(5, 6, state=st, **kw), m.generate(5, 6, state=copy, **kw)
    assert same(a, b) and same_state(st, copy)
    third = m.new_state(5, history=7)
    m.feed(third, songs)
    assert same(m.generate(5, 6, state=third, **kw), a) and same_state(st, third)
    # n_ctx = 0 through set: the start word is pending, as in a fresh state
    z = np.zeros((L, 5, H), np.float32)
    copy.set(z, z)
    third.reset()
    assert same(m.generate(5, 4, state=copy, **kw), m.generate(5, 4, state=third, **kw))
    for s in (st, copy, third):
        s.close()


def test_feed_kernel_staged_row_at_full_size():
    # V1 = 10 001 (staged in LDS), hidden 512, 8 positions
    m, cfg = _trained(steps=1, input_size=10000, max_len=8, embedding_size=32, hidden_size=512)
    x = _primer(3, 8, seed=1, vocab=10001)
    st = m.new_state(3, history=8)
    lp = m.feed(st, x, logprobs=True)
    ref = D.State(f64_params(m), cfg, 3, 8).feed(x, logprobs=True)
    err = np.abs(lp - ref).max()
    print('max abs err', err)
    assert err <= 1e-4
    toks, lps = m.generate(3, 8, temperature=1.0, seed=2, logprobs=True, state=st)
    again = m.new_state(3, history=8)
    m.feed(again, x)
    assert same((m.feed(again, toks, logprobs=True),), (lps,))
    st.close()
    again.close()


def test_feed_kernel_unstaged_row_with_the_penalty():
    # V1 = 50 001: the row is read from global memory, the pick keeps the penalty's presence bitmap in LDS
    m, cfg = _trained(steps=1, input_size=50000, max_len=8, embedding_size=8, hidden_size=24)
    kw = dict(temperature=0.8, top_k=40, repetition_penalty=1.4, repeat_window=4, seed=5, logprobs=True)
    primer = _primer(3, 2, seed=4, vocab=50000)
    want = m.generate(3, 6, primer=primer, **kw)
    st = m.new_state(3, history=4)
    m.feed(st, primer)
    a, b = m.generate(3, 2, state=st, **kw), m.generate(3, 4, state=st, **kw)
    assert same((np.concatenate([a[0], b[0]], 1), np.concatenate([a[1], b[1]], 1)), want)
    again = m.new_state(3, history=4)
    lp = m.feed(again, np.concatenate([primer, want[0]], 1), logprobs=True)
    assert same((lp[:, 2:],), (want[1],))
    ref = D.State(f64_params(m), cfg, 3, 4).feed(np.concatenate([primer, want[0]], 1), logprobs=True)
    err = np.abs(lp - ref).max()
    print('max abs err', err)
    assert err <= 1e-4
    st.close()
    again.close()


def test_chunked_run_against_fp64_margins():
    m, cfg = _trained(**TWO_LAYER)
    primer = _primer(4, 3, seed=6)
    st = m.new_state(4, history=8)
    m.feed(st, primer)
    chunks = [m.generate(4, n, temperature=0.8, top_k=6, seed=17, logprobs=True, state=st) for n in (5, 1, 6)]
    toks, lps = np.concatenate([c[0] for c in chunks], 1), np.concatenate([c[1] for c in chunks], 1)
    R.check_margins(f64_params(m), cfg, toks, lps, 0.8, 6, 17, primer=primer, tol=1e-4, tie=1e-4)
    st.close()


def test_feed_logprobs_against_score_and_a_long_song_in_chunks():
    m, cfg = _trained(**TWO_LAYER)
    T = cfg['max_len']
    songs = _primer(6, T, seed=8)
    st = m.new_state(6, history=4)
    lp = m.feed(st, songs, logprobs=True)
    score = m.score(songs)['logprob']
    err = np.abs(lp.astype(np.float64) - score).max()
    print('feed against fsmg_score: max abs diff', err)
    assert err <= 2e-4          # two kernel families, each within 1e-4 of fp64
    # a song of 3 x max_len tokens, which fsmg_score cannot read, in three chunks
    long_song = _primer(2, 3 * T, seed=10)
    st2 = m.new_state(2, history=4)
    got = np.concatenate([m.feed(st2, long_song[:, i * T:(i + 1) * T], logprobs=True) for i in range(3)], 1)
    ref = D.State(f64_params(m), cfg, 2, 4).feed(long_song, logprobs=True)
    err = np.abs(got - ref).max()
    print('3 x max_len against fp64: max abs err', err)
    assert err <= 1e-4
    assert st2.info()['n_ctx'] == 3 * T
    st.close()
    st2.close()


def test_e6_beam_search_from_a_state():
    m, cfg = _trained(**SMALL)
    primer = _primer(2, 4, seed=11)
    want = m.beam_search(6, 3, n_groups=2, primer=primer, logprobs=True)
    st = m.new_state(2, history=8)
    m.feed(st, primer)
    before = st.get()
    got = m.beam_search(6, 3, n_groups=2, logprobs=True, state=st)
    assert same(got, want)
    after = st.get()                                    # read, not modified
    assert same((before['h'], before['c'], before['ctx']), (after['h'], after['c'], after['ctx']))
    assert (after['n_ctx'], after['n_gen']) == (4, 0)
    st.close()


def _handle_state(m):
    opt = {k: m.get_opt_state(k) for k in m.param_shapes}
    return m.get_params(), opt, m.step, m.read_losses(2), m.stats(), {k: m.get_grad(k) for k in m.param_shapes}


def test_e7_no_handle_state_changes_and_e8_one_shot_bits_stay():
    cfg = small_config(**SMALL)
    m = new_model(cfg)
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, cfg['max_len'], cfg['input_size'], seed=7):
        m.train_step(sup, qry)
    primer = _primer(3, 4)
    one_shot = m.generate(3, 7, seed=21, primer=primer, logprobs=True, **FILTERED)
    beam = m.beam_search(5, 2, n_groups=3, primer=primer, logprobs=True)
    before = _handle_state(m)
    st, dst = m.new_state(3, history=8), m.new_state(2, history=8)
    m.feed(st, primer, logprobs=True)
    m.generate(3, 5, seed=1, state=st, **FILTERED)
    m.beam_search(4, 2, n_groups=3, state=st)
    dst.gather(st, [2, 0])
    g = st.get()
    st.set(g['h'], g['c'], g['ctx'], g['n_ctx'], g['n_gen'])
    st.reset()
    st.close()
    dst.close()
    after = _handle_state(m)
    for k in before[0]:
        assert np.array_equal(bits(before[0][k]), bits(after[0][k])), k
        assert np.array_equal(before[1][k][0], after[1][k][0]) and np.array_equal(before[1][k][1], after[1][k][1]), k
        assert np.array_equal(bits(before[5][k]), bits(after[5][k])), k
    assert before[2] == after[2] and np.array_equal(before[3], after[3]) and before[4] == after[4]
    # the one-shot entry points after stateful calls: the bits they returned before
    assert same(m.generate(3, 7, seed=21, primer=primer, logprobs=True, **FILTERED), one_shot)
    assert same(m.beam_search(5, 2, n_groups=3, primer=primer, logprobs=True), beam)
    m.close()


def test_argument_errors():
    from fsmg.binding import FsmgDstateConfig, FsmgError, FsmgModel
    import torch
    m, cfg = _trained(**SMALL)
    lib, V = m._lib, cfg['input_size']

    def create(**over):
        c = FsmgDstateConfig(version=1, n_rows=2, history=4)
        for k, v in over.items():
            if k == 'reserved':
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        out = C.c_void_p()
        rc = lib.fsmg_dstate_create(m._h, C.byref(c), C.byref(out))
        if rc == 0:
            assert lib.fsmg_dstate_destroy(m._h, out) == 0
        return rc

    assert create() == 0
    for bad in (dict(version=2), dict(reserved=0), dict(reserved=8), dict(n_rows=0), dict(n_rows=-3), dict(history=0),
                dict(n_rows=(1 << 20) + 1)):
        assert create(**bad) == -1, bad

    st = m.new_state(2, history=4)
    out_t = np.empty((2, 8), np.int32)
    out_s = np.empty((2, 2), np.float32)
    tp = out_t.ctypes.data_as(_I32P)

    def gen(**over):
        g = m.gen_config(2, 3, 1.0, 0, 0)
        for k, v in over.items():
            setattr(g, k, v)
        return lib.fsmg_dstate_generate(m._h, st._st, C.byref(g), None, tp, None)

    def beam(**over):
        b = m.beam_config(2, 2, 3)
        for k, v in over.items():
            setattr(b, k, v)
        return lib.fsmg_dstate_beam_search(m._h, st._st, C.byref(b), tp, out_s.ctypes.data_as(C.POINTER(C.c_float)), None)

    untouched = st.get()
    # row-count mismatches, a primer_len, everything the one-shot calls refuse
    for bad in (dict(n_seq=3), dict(n_seq=1), dict(primer_len=1), dict(version=2), dict(num=-1), dict(temperature=-1.0),
                dict(top_k=V + 2), dict(num=1 << 30)):
        assert gen(**bad) == -1, bad
    for bad in (dict(n_groups=3), dict(primer_len=2), dict(beam_width=65), dict(beam_width=0), dict(num=0), dict(version=0)):
        assert beam(**bad) == -1, bad
    # feed: n < 0, a bad flag, too many token slots (refused before the tokens are read)
    x = np.zeros((2, 3), np.int32)
    xp = C.c_void_p(x.ctypes.data)
    assert lib.fsmg_dstate_feed(m._h, st._st, xp, -1, 0, None) == -1
    assert lib.fsmg_dstate_feed(m._h, st._st, xp, 3, 2, None) == -1
    assert lib.fsmg_dstate_feed(m._h, st._st, None, 3, 0, None) == -1
    assert lib.fsmg_dstate_feed(m._h, st._st, xp, 1 << 29, 0, None) == -1          # 2 * (4 + 2^29 + 1) > 2^30
    assert lib.fsmg_dstate_feed(m._h, st._st, xp, 0, 0, None) == 0                 # nothing to read: a no-op
    # token range: host tokens before any device work (the state stays), the start word is allowed
    for bad in (V + 1, -1):
        x[1, 2] = bad
        with pytest.raises(FsmgError) as e:
            m.feed(st, x)
        assert e.value.code == -7
    after = st.get()
    assert same((untouched['h'], untouched['c']), (after['h'], after['c'])) and st.info()['n_ctx'] == 0
    x[1, 2] = V
    m.feed(st, x)
    assert st.info()['n_ctx'] == 3
    # device tokens: the flag comes back with the outputs; afterwards the state is unspecified but usable once reset
    d_ok = torch.tensor(x, dtype=torch.int32, device='cuda')
    st.reset()
    host_lp = m.feed(st, x, logprobs=True)
    st.reset()
    assert same((m.feed(st, (d_ok.data_ptr(), 3), logprobs=True),), (host_lp,))
    d_bad = d_ok.clone()
    d_bad[0, 1] = V + 1
    for lp in (False, True):
        with pytest.raises(FsmgError) as e:
            m.feed(st, (d_bad.data_ptr(), 3), logprobs=lp)
        assert e.value.code == -7
    st.reset()
    assert same((m.feed(st, x, logprobs=True),), (host_lp,))
    # set: shapes on the device side of the boundary, ctx ids, counters
    g = st.get()
    with pytest.raises(FsmgError) as e:
        st.set(g['h'], g['c'], np.full((2, 3), V + 1, np.int32), 3, 0)
    assert e.value.code == -7
    for n_ctx, n_gen in ((3, 4), (-1, 0), (3, -1)):
        with pytest.raises(FsmgError) as e:
            st.set(g['h'], g['c'], g['ctx'][:, :max(min(n_ctx, 4), 0)], n_ctx, n_gen)
        assert e.value.code == -1
    assert lib.fsmg_dstate_set(m._h, st._st, None, None, None, 0, 0) == -1
    assert lib.fsmg_dstate_set(m._h, st._st, g['h'].ctypes.data_as(C.POINTER(C.c_float)), g['c'].ctypes.data_as(C.POINTER(C.c_float)),
                               None, 3, 0) == -1
    # gather: an index out of range, dst == src, unequal histories
    other, wide = m.new_state(3, history=4), m.new_state(3, history=5)
    for rows in ([0, 1, 2], [0, -1, 0]):
        with pytest.raises(FsmgError) as e:
            other.gather(st, rows)
        assert e.value.code == -1
    other.gather(st, [1, 1, 0])
    idx = np.zeros(3, np.int32)
    assert lib.fsmg_dstate_gather(m._h, other._st, other._st, idx.ctypes.data_as(_I32P)) == -1
    assert lib.fsmg_dstate_gather(m._h, other._st, st._st, None) == -1
    with pytest.raises(FsmgError) as e:
        wide.gather(other, [0, 1, 2])
    assert e.value.code == -1
    # a destroyed state and another handle's state: the registry says no
    gone = C.c_void_p(wide._st.value)
    wide.close()
    m2 = FsmgModel(cfg)
    foreign = m2.new_state(2, history=4)
    info = (C.c_int64 * 4)()
    for ptr in (gone, foreign._st, C.c_void_p(None)):
        assert lib.fsmg_dstate_destroy(m._h, ptr) == -1
        assert lib.fsmg_dstate_reset(m._h, ptr) == -1
        assert lib.fsmg_dstate_info(m._h, ptr, info) == -1
        assert lib.fsmg_dstate_get(m._h, ptr, None, None, None) == -1
        assert lib.fsmg_dstate_feed(m._h, ptr, xp, 3, 0, None) == -1
        assert lib.fsmg_dstate_gather(m._h, ptr, st._st, idx.ctypes.data_as(_I32P)) == -1
        assert lib.fsmg_dstate_gather(m._h, other._st, ptr, idx.ctypes.data_as(_I32P)) == -1
        g2 = m.gen_config(2, 3, 1.0, 0, 0)
        assert lib.fsmg_dstate_generate(m._h, ptr, C.byref(g2), None, tp, None) == -1
    assert 'decode state' in lib.fsmg_last_error(m._h).decode()
    assert foreign.info()['rows'] == 2                  # the other handle's state is alive and well
    # fsmg_destroy with live states frees them; closing such a state afterwards is a no-op
    m2.close()
    foreign.close()
    st.close()
    other.close()
    assert m.generate(1, 2, temperature=0.0).shape == (1, 2)


def _episode(cfg, N=2, K=2, Q=2, seed=3):
    rs = np.random.RandomState(seed)
    T, V = cfg['max_len'], cfg['input_size']

    class Episode(object):
        support = rs.randint(0, V, size=(N, K, T)).astype(np.int32)
        query = rs.randint(0, V, size=(N, Q, T)).astype(np.int32)
    return Episode


def _plugin(tmp_path, **over):
    from models.lstm_baseline import LSTMBaseline
    cfg = dict(small_config(input_size=40, max_len=12, embedding_size=8, hidden_size=16), name='lstm_baseline', checkpt_dir=str(tmp_path))
    cfg.update(over)
    model = LSTMBaseline(cfg)
    model.recover_or_init('')
    for sup, qry in O.synthetic_episodes(3, 2, 2, 2, 12, 40, seed=2):
        model.engine.train_step(sup, qry)
    return model, cfg


def test_plugin_condition_and_eval_conditioned(tmp_path):
    model, cfg = _plugin(tmp_path)
    ep = _episode(cfg)
    params = f64_params(model.engine)
    state = model.condition(ep.support)
    want = D.condition(params, cfg, ep.support)
    got = state.get()
    assert state.rows == 2 and (got['n_ctx'], got['n_gen']) == (want.n_ctx, 0) and got['n_ctx'] == 2 * 12 + 1
    h, c, ctx = want.arrays()
    assert got['ctx'].tolist() == ctx.tolist()
    assert np.abs(got['h'] - h).max() <= 2e-5 * np.abs(h).max() and np.abs(got['c'] - c).max() <= 2e-5 * np.abs(c).max()
    state.close()
    nll = model.eval_conditioned(ep)
    ref = D.eval_conditioned(params, cfg, ep.support, ep.query)
    print('eval_conditioned', nll, 'fp64', ref, 'eval', model.eval(ep))
    assert abs(nll - ref) <= 1e-4 * abs(ref)
    assert abs(nll - model.eval(ep)) > 1e-4             # the support set is really read (fp32 noise of a mean NLL: ~1e-6)
    assert model.engine.step == 3                       # and nothing was trained


def test_plugin_generate_conditioned_on_support(tmp_path):
    model, cfg = _plugin(tmp_path)
    support = _episode(cfg).support[0]                  # [K, T], what train.train passes
    kw = dict(n=3, temperature=1.0, top_k=8, seed=5, primer_len=2, repetition_penalty=1.2)
    a = model.generate(support, 9, condition_on_support=True, **kw)
    assert a.shape == (3, 9) and a.dtype == np.int32 and np.all((a >= 0) & (a <= 40))
    assert np.array_equal(a, model.generate(support, 9, condition_on_support=True, **kw))
    assert not np.array_equal(a, model.generate(support, 9, **kw))
    # by hand on the engine: one long primer per row [song_1, start, song_2, start, primer]
    eng, K, T = model.engine, 2, 12
    st = eng.new_state(3, history=K * (T + 1) + 1 + 2 + 9)
    start = np.full((3, 1), 40, np.int32)
    rows = np.arange(3) % K
    eng.feed(st, np.concatenate([np.tile(support[0], (3, 1)), start, np.tile(support[1], (3, 1)), start, support[rows, :2]], 1))
    b = eng.generate(3, 9, temperature=1.0, top_k=8, seed=5, repetition_penalty=1.2, state=st)
    assert np.array_equal(a, b)
    # two artists: row i continues artist i % 2 and a primer from that artist's own songs
    both = _episode(cfg).support
    c = model.generate(both, 9, condition_on_support=True, **kw)
    artist, song = np.arange(3) % 2, (np.arange(3) // 2) % K
    st.reset()
    eng.feed(st, np.concatenate([both[artist, 0], start, both[artist, 1], start, both[artist, song, :2]], 1))
    assert np.array_equal(c, eng.generate(3, 9, temperature=1.0, top_k=8, seed=5, repetition_penalty=1.2, state=st))
    st.close()


def test_train_entry_condition_key(tmp_path, golden_dir):
    import test_train_entry as E
    import train.train as T
    base = dict(E.LOOP, name='lstm_baseline', model_module_name='models.lstm_baseline', model_class_name='LSTMBaseline', seed=1,
                embedding_size=8, hidden_size=16, n_layers=1, lr=1e-3, max_grad_norm=5, n_decay=1000,
                sample_temperature=1.0, sample_top_k=10, sample_seed=4, samples_per_episode=2)
    texts = {}
    for name, extra in (('plain', {}), ('off', dict(sample_condition_on_support=False)), ('on', dict(sample_condition_on_support=True))):
        tmp = tmp_path / name
        tmp.mkdir()
        p = E._write_configs(tmp, golden_dir, dict(base, **extra))
        ck = str(tmp / 'ck')
        T.main(['--data', p['data'], '--task', p['task'], '--model', p['model'], '--checkpt_dir', ck])
        texts[name] = {}
        for i in range(base['n_samples']):
            d = os.path.join(ck, 'samples', 'sample_%d' % i)
            assert sorted(os.listdir(d)) == ['model_sample_0.txt', 'model_sample_1.txt'] + ['support_%d.txt' % j for j in range(E.K)]
            for f in os.listdir(d):
                texts[name][(i, f)] = open(os.path.join(d, f), 'rb').read()
    assert texts['plain'] == texts['off']               # without the key every written file is what it was
    sup = {k: v for k, v in texts['on'].items() if k[1].startswith('support')}
    assert sup == {k: v for k, v in texts['plain'].items() if k[1].startswith('support')}
    gen_on = {k: v for k, v in texts['on'].items() if k[1].startswith('model_sample')}
    assert all(len(v) > 0 for v in gen_on.values())
    assert gen_on != {k: v for k, v in texts['plain'].items() if k[1].startswith('model_sample')}
