"""The componentwise measure of tests/backward_ref.py with per-row weights -- the padding-masked pass -- on the CPU
alone: the weighted restatement is tests/masked_ref.py's bit for bit and the unweighted one at full lengths, it obeys the padding law
itself, and the measure sees planted errors of the kind masking invites, which the whole-tensor bounds of tests/test_masked.py
(max|err| / max|ref| < 2e-4 on the gradients) let through.

Every planted error is applied to the fp64 reference itself, so what is tested is the measure, not a kernel.
"""
import numpy as np
import pytest

import backward_ref as R
import masked_ref as MR
from conftest import small_config
from gpu_utils import rel_max
from oracle import lstm_oracle as O

REL_MAX_BAR = 2e-4          # the whole-tensor gradient bound of tests/test_masked.py
M = 8                       # the device's bound is M * e32; a planted error must miss it by a factor of 10 at least

_REFS = {}


def case(shape):
    """-> cfg, (sup, qry), (support_len, query_len), lengths [B] in the pass's row order"""
    over, N, K, Q, seed = shape
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    sl, ql = MR.componentwise_lengths(cfg, N, K, Q, seed)
    return cfg, (sup, qry), (sl, ql), MR.train_lengths(sl, ql)


def reference(shape):
    """the weighted Reference of one shape from the device's tokens (MR.device_xy): computed once, never written to"""
    key = R.shape_id(shape) + '/%d' % shape[4]
    if key not in _REFS:
        cfg, (sup, qry), (sl, ql), ln = case(shape)
        X, Y = MR.device_xy(sup, qry, sl, ql, cfg)
        _REFS[key] = (cfg, ln, R.Reference(O.glorot_init(cfg, 0), X, Y, cfg, weights=MR.mask_of(ln, cfg['max_len'])))
    return _REFS[key]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ----------------------------------------------------------------------------- the references agree, in fp64
@pytest.mark.parametrize('layers', [1, 2])
def test_weighted_restatement_is_masked_ref_bit_for_bit(layers):
    cfg = small_config(hidden_size=20, embedding_size=10, input_size=50, max_len=7, n_layers=layers)
    sup, qry = R.episode(cfg, 2, 2, 1, 3)
    sl, ql = MR.componentwise_lengths(cfg, 2, 2, 1, 3)
    ln = MR.train_lengths(sl, ql)
    assert ln.min() == 1 and ln.max() == 7 and len(set(ln.tolist())) > 2
    params = O.glorot_init(cfg, 1)
    loss, cache, grads, aux = MR.step(params, sup, qry, sl, ql, cfg)
    full = R.backward_full(params, cache, cfg, weights=MR.mask_of(ln, 7))
    assert sorted(full['grads']) == sorted(grads)
    for k in grads:
        assert _bits_equal(full['grads'][k], grads[k]), k
    assert full['aux'] == aux
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    assert R.Reference(params, X, Y, cfg, weights=MR.mask_of(ln, 7)).loss == loss
    # a masked row: S == 0 in dlogits, dh, dx, zeros in dz; a scored row: S > 0 in every element
    masked = MR.mask_of(ln, 7) == 0
    assert masked.any() and not masked.all()
    for name in ('dlogits', 'dh', 'dx'):
        S = full['scales'][name]
        assert np.all(S[masked] == 0) and np.all(S[~masked] > 0), name
        assert np.all(full[name][masked] == 0), name
    for dz in full['dz']:
        assert np.all(dz[masked] == 0) and np.all(np.abs(dz[~masked]).max(axis=1) > 0)
    for k, S in full['scales'].items():
        assert np.all(S >= 0) and np.all(np.isfinite(S)), k


@pytest.mark.parametrize('layers', [1, 2])
def test_full_lengths_are_the_unweighted_restatement_bit_for_bit(layers):
    cfg = small_config(hidden_size=20, embedding_size=10, input_size=50, max_len=7, n_layers=layers)
    sup, qry = R.episode(cfg, 2, 2, 1, 3)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    params = O.glorot_init(cfg, 1)
    _, cache = O.forward(params, X, Y, cfg)
    a = R.backward_full(params, cache, cfg)
    b = R.backward_full(params, cache, cfg, weights=np.ones(X.size))
    assert a['aux'] == b['aux']
    for k in a['grads']:
        assert _bits_equal(a['grads'][k], b['grads'][k]), k
    for k in a['scales']:
        assert _bits_equal(a['scales'][k], b['scales'][k]), k
    for k in ('dlogits', 'dx', 'dh'):
        assert _bits_equal(a[k], b[k]), k
    for x, y in zip(a['dz'], b['dz']):
        assert _bits_equal(x, y)
    # ... and the two References: the loss, every tensor, every e32
    ra, rb = R.Reference(params, X, Y, cfg), R.Reference(params, X, Y, cfg, weights=np.ones(X.size))
    assert ra.loss == rb.loss and ra.e32 == rb.e32
    for k in ra.t:
        assert _bits_equal(ra.t[k], rb.t[k]), k
    # the full-length device tokens are the oracle's
    T = cfg['max_len']
    Xd, Yd = MR.device_xy(sup, qry, np.full((2, 2), T), np.full((2, 1), T), cfg)
    assert np.array_equal(Xd, X) and np.array_equal(Yd, Y)


def test_the_reference_obeys_the_padding_law_itself():
    """gradients from the caller's tokens, from other tokens behind the songs' ends, and from the device's fixed ids there"""
    cfg = small_config(n_layers=2, hidden_size=12)
    N, K, Q = 3, 2, 2
    sup, qry = R.episode(cfg, N, K, Q, 5)
    sl, ql = MR.componentwise_lengths(cfg, N, K, Q, 5)
    ln = MR.train_lengths(sl, ql)
    rng = np.random.RandomState(6)
    sup2, qry2 = MR.scramble_padding(sup, sl, cfg['input_size'], rng), MR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) and not np.array_equal(qry, qry2)
    params = O.glorot_init(cfg, 9)
    w = MR.mask_of(ln, cfg['max_len'])
    tokens = [O.train_xy(sup, qry, cfg['input_size']), O.train_xy(sup2, qry2, cfg['input_size']), MR.device_xy(sup, qry, sl, ql, cfg)]
    assert np.array_equal(MR.device_xy(sup2, qry2, sl, ql, cfg)[0], tokens[2][0])
    assert not np.array_equal(tokens[0][0], tokens[2][0]) and not np.array_equal(tokens[0][1], tokens[2][1])
    pad = w.reshape(ln.size, -1) == 0
    assert np.all(tokens[2][0][pad] == cfg['input_size']) and np.all(tokens[2][1][pad] == 0)
    assert np.array_equal(tokens[2][0][~pad], tokens[0][0][~pad]) and np.array_equal(tokens[2][1][~pad], tokens[0][1][~pad])
    fulls = []
    for X, Y in tokens:
        _, cache = O.forward(params, X, Y, cfg)
        fulls.append(R.backward_full(params, cache, cfg, weights=w))
    for other in fulls[1:]:
        assert other['aux'] == fulls[0]['aux']
        for k in fulls[0]['grads']:
            assert np.array_equal(other['grads'][k], fulls[0]['grads'][k]), k
        for k in ('softmax_w', 'softmax_b', 'kernel_0', 'kernel_1', 'bias_0', 'bias_1', 'embedding', 'dlogits', 'dh', 'dx'):
            assert np.array_equal(other['scales'][k], fulls[0]['scales'][k]), k


# ----------------------------------------------------------------------------- the lengths of every shape
@pytest.mark.parametrize('shape', R.CW_SHAPES, ids=R.shape_id)
def test_lengths_of_every_shape_hold_the_edges(shape):
    cfg, (sup, qry), (sl, ql), ln = case(shape)
    T, B = cfg['max_len'], ln.size
    assert ln.min() == 1 and ln.max() == T
    if B >= 3 and T >= 3:
        assert ((ln > 1) & (ln < T)).any()
    mask = MR.mask_of(ln, T).reshape(B, T)
    assert (mask == 0).any() and (mask == 1).any()                # one masked and one scored row at least
    assert mask.mean() >= 0.25, mask.mean()                       # a quarter of the rows is scored
    if B >= 32:
        late = mask[:, T // 2:]
        assert not late[16:32].any()                              # a whole 16-row tile of the recurrence masked in the late steps ...
        for tile in (late[0:16], late[32:48]):                    # ... between mixed ones
            assert tile.any() and not tile.all()
    assert np.array_equal(MR.train_lengths(*MR.componentwise_lengths(cfg, *shape[1:])), ln)          # seeded
    X, _ = MR.device_xy(sup, qry, sl, ql, cfg)
    if T == 96:       # the two-level embedding gradient sums the start word, most of whose terms are zeros
        assert (X == cfg['input_size']).sum() > 48


def expected_zero_share(cfg, X, ln):
    """the share of elements with S == 0 per family, from the tokens and the lengths alone: a masked row of dlogits, dh, dx; an
    embedding row whose token is no input at or before a scored position (behind it BPTT carries nothing); nothing else, as
    long as some song is longer than 1 (h_-1 = c_-1 = 0 would empty the recurrent rows and the forget gate otherwise)"""
    T = cfg['max_len']
    assert ln.max() > 1
    mask = MR.mask_of(ln, T)
    row_share = float((mask == 0).mean())
    live = np.unique(X.reshape(-1)[mask == 1])
    share = dict(logits=0.0, lse=0.0, ce=0.0, dlogits=row_share, dh=row_share, dx=row_share, softmax_w=0.0, softmax_b=0.0, kernel=0.0, bias=0.0,
                 embedding=1.0 - live.size / float(cfg['input_size'] + 1))
    return share


@pytest.mark.parametrize('shape', R.CW_SHAPES, ids=R.shape_id)
def test_exact_zero_elements_are_no_more_than_the_lengths_explain(shape):
    """an element with S == 0 is held to exact zero and not to the bound: no family may hide more of its elements there than the
    masked rows and the absent tokens account for -- and the reference holds itself inside the bound it sets"""
    cfg, ln, ref = reference(shape)
    want = expected_zero_share(cfg, ref.X, ln)
    assert sorted(ref.e32) == sorted(R.FAMILIES)
    for fam, e in ref.e32.items():
        assert np.isfinite(e) and 1e-8 < e < 1e-4, (fam, e)
    masked = MR.mask_of(ln, cfg['max_len']) == 0
    for (fam, layer), ref_t in ref.t.items():
        assert not ref.failures(fam, layer, ref_t, M).any()
        if fam in R.SLICEWISE:
            continue
        S = R.scale_of(ref.full, fam, layer)
        got = float((S == 0).mean())
        print('ZERO|%s|%s%s|%d of %d|share %.4f|explained %.4f' % (R.shape_id(shape), fam, '' if layer is None else layer,
                                                                  int((S == 0).sum()), S.size, got, want[fam]))
        assert got <= want[fam] + 1e-12, (fam, layer, got, want[fam])
        if fam in ('dlogits', 'dh', 'dx'):
            assert np.all(S[masked] == 0) and np.all(S[~masked] > 0), fam
    for l in range(cfg['n_layers']):
        dz = ref.t[('dz', l)].reshape(masked.size, -1)
        assert np.all(dz[masked] == 0) and np.all(np.abs(dz[~masked]).max(axis=1) > 0)


# ----------------------------------------------------------------------------- planted errors
MUTANT_SHAPE = R.CW_SHAPES[2]           # B = 45, T = 9, vocabulary 301


def miss(ref, fam, layer, planted):
    """by how many times the worst element (slice) of `planted` misses the device's bound M * e32 * S + 1e-30 -- the inequality
    of Reference.failures; where S == 0 (a zero slice) that is |planted| / 1e-30"""
    tol = M * ref.e32[fam]
    want = ref.t[(fam, layer)]
    if fam in R.SLICEWISE:
        axes = R.SLICE_AXES[fam]
        err, den = np.abs(planted - want).max(axis=axes), np.abs(want).max(axis=axes)
    else:
        err, den = np.abs(planted - want), R.scale_of(ref.full, fam, layer)
    return float((err / (tol * den + R.UNDERFLOW)).max())


def _seen(name, ref, fam, layer, planted, n_bad=None):
    want = ref.t[(fam, layer)]
    old, new = rel_max(planted, want), miss(ref, fam, layer, planted)
    bad = ref.failures(fam, layer, planted, M)
    print('MUTANT|%s|%s|max|err| / max|ref| = %.2e (bar %.0e)|misses M * e32 * S by %.3g x|%d elements outside' % (
        name, fam, old, REL_MAX_BAR, new, int(bad.sum())))
    assert not ref.failures(fam, layer, want, M).any()
    assert old < REL_MAX_BAR, (name, old)                # the old measure passes it
    assert new >= 10, (name, new)
    assert bad.sum() == n_bad if n_bad is not None else bad.any(), (name, int(bad.sum()))


def test_a_leaking_masked_row_of_dlogits_is_seen():
    cfg, ln, ref = reference(MUTANT_SHAPE)
    T = cfg['max_len']
    b = int(np.argmin(ln))
    r = b * T + T - 1                                   # the last position of the shortest song: masked
    assert ln[b] < T and ref.weights[r] == 0 and np.all(ref.t[('dlogits', None)][r] == 0)
    unmasked = R.backward_full(ref.params, ref.cache, cfg)['dlogits'][r] * (ln.size * T) / float(ln.sum())       # the row with weight 1 / n_valid
    planted = ref.t[('dlogits', None)].copy()
    planted[r] = 1e-5 * unmasked
    _seen('leak 1e-5 of a masked dlogits row', ref, 'dlogits', None, planted, n_bad=planted.shape[1])
    # ... and what the leak does to the gradients it flows into stays far below the old bar as well
    for name, g in (('softmax_w', ref.cache['out'].T.dot(planted)), ('softmax_b', planted.sum(axis=0))):
        old = rel_max(g, ref.t[(name, None)])
        print('MUTANT|the same leak in %s|max|err| / max|ref| = %.2e|%.3g x M * e32 * S' % (name, old, miss(ref, name, None, g)))
        assert old < REL_MAX_BAR


def test_an_embedding_row_of_a_token_behind_the_songs_ends_is_seen():
    """the caller's tokens: a token that sits only behind songs' ends is an input of the oracle's pass and must get exact zeros"""
    cfg, (sup, qry), (sl, ql), ln = case(MUTANT_SHAPE)
    T = cfg['max_len']
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    ref = R.Reference(O.glorot_init(cfg, 0), X, Y, cfg, weights=MR.mask_of(ln, T))
    scored = MR.mask_of(ln, T).reshape(X.shape) == 1
    only_behind = np.setdiff1d(np.unique(X[~scored]), np.unique(X[scored]))
    assert only_behind.size > 0
    g, S = ref.t[('embedding', None)], ref.full['scales']['embedding']
    assert np.all(S[only_behind] == 0) and np.all(g[only_behind] == 0) and np.all(S[np.unique(X[scored])] > 0)
    # the device's tokens give the same gradient: the start word's extra terms are zeros
    _, _, dev = reference(MUTANT_SHAPE)
    assert np.array_equal(dev.t[('embedding', None)], g)
    planted = g.copy()
    planted[only_behind[0]] = 1e-6 * np.abs(g).max()
    _seen('1e-6 of the maximum in the row of a token behind the ends', ref, 'embedding', None, planted, n_bad=g.shape[1])


def test_a_dropped_last_scored_position_of_the_shortest_song_is_seen():
    cfg, ln, ref = reference(MUTANT_SHAPE)
    T = cfg['max_len']
    b = int(np.argmin(ln))
    r = b * T + int(ln[b]) - 1
    dl = ref.t[('dlogits', None)]
    assert ref.weights[r] == 1 and (ln[b] == T or ref.weights[r + 1] == 0)
    c = int(np.argmin(np.abs(dl[r])))                    # a rare column: never this row's target
    assert c != ref.Y.reshape(-1)[r] and dl[r, c] != 0
    planted = ref.t[('softmax_b', None)].copy()
    planted[c] -= dl[r, c]
    _seen('t = len - 1 of the shortest song dropped from a rare column of softmax_b', ref, 'softmax_b', None, planted, n_bad=1)


def test_a_nonzero_masked_row_of_dz_is_seen():
    cfg, ln, ref = reference(MUTANT_SHAPE)
    T = cfg['max_len']
    b = int(np.argmin(ln))
    dz = ref.t[('dz', 0)]                                # [B, T, gate, H]
    assert np.all(dz[b, T - 1] == 0)
    planted = dz.copy()
    planted[b, T - 1] = 1e-6 * np.abs(dz).max()
    _seen('1e-6 of the maximum in a masked (t, b) row of dz', ref, 'dz', 0, planted, n_bad=4)
