"""-m gpu: the padding-masked train pass against the fp64 oracle ELEMENT BY ELEMENT, and the masked eval relative to
its own value.

tests/test_masked.py holds the masked step to max|err| / max|ref| per gradient and to its two laws through the gradients; what
tests/test_gpu_componentwise.py says about that measure holds more sharply under a mask, where whole rows of dlogits, dh, dx and of
every dz must be exact zeros beside rows that are not (tests/test_masked_componentwise_cpu.py plants the errors it lets through).
Here the measure of tests/backward_ref.py with the rows' weights:

  * the reference is built from the DEVICE's tokens (masked_ref.device_xy: start word / 0 behind a song's end), so hs, cs, logits,
    lse and ce are compared on all rows, the masked ones included;
  * an element with S == 0 -- every element of a masked row of dlogits, dh, dx, the embedding row of a token that is an input only
    behind songs' ends -- must be exactly 0.0 (-0.0 counts), and so must every masked (t, b) row of dz;
  * everything else is held to M * e32 with the M = 8 of the unmasked pass, e32 from the weighted fp32 restatement of the shape.

The lengths are masked_ref.componentwise_lengths': seeded, with a 1, a T, a value between, and -- from 32 rows on -- rows 16 .. 31 no
longer than T // 2, so that one whole 16-row tile of the recurrence is masked in the late steps between mixed ones
(tests/test_masked_componentwise_cpu.py checks these properties and the quarter of scored rows for every shape).  The measured
err / (S * e32) of every shape, GEMM kind and family is recorded in tests/COMPONENTWISE.md, "The masked pass".
"""
import os

import numpy as np
import pytest

import backward_ref as R
import masked_ref as MR
from conftest import small_config
from gpu_utils import f64_params, new_model
from oracle import lstm_oracle as O
from test_gpu_componentwise import FUSED, M, check_all, device_tensors

pytestmark = pytest.mark.gpu

assert M == 8           # the project's constant: not this file's to raise
U = 2.0 ** -24

# one shape per recurrence family: the default, the persistent chain (H 128), the slice kernels (H 256), the XCD-local kernels in
# fp32 (H 512, 45 rows) and bf16-split (H 512, 100 rows), the stacked pair kernels (H 1024, 2 layers)
FAMILY_SHAPES = [R.CW_SHAPES[i] for i in (0, 4, 6, 7, 8, 9)]
assert [s[0].get('hidden_size') for s in FAMILY_SHAPES] == [None, 128, 256, 512, 512, 1024]


@pytest.fixture(params=['bx3', 'f32'])
def gemm_kind(request, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', request.param)
    return request.param


def case(shape, all_ones=False):
    """-> cfg, (sup, qry), (support_len, query_len), lengths [B] in the pass's row order"""
    over, N, K, Q, seed = shape
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    sl, ql = MR.componentwise_lengths(cfg, N, K, Q, seed)
    if all_ones:
        sl, ql = np.ones_like(sl), np.ones_like(ql)
    return cfg, (sup.astype(np.int32), qry.astype(np.int32)), (sl, ql), MR.train_lengths(sl, ql)


_REFS = {}


def reference(key, model, sup, qry, sl, ql, cfg):
    """fp64 oracle + fp32 restatement of one masked pass from the device's tokens: computed once per key, shared by the cases that
    run the same shape and lengths (same seeded parameters -- asserted), never written to"""
    params = f64_params(model)
    if key not in _REFS:
        X, Y = MR.device_xy(sup, qry, sl, ql, cfg)
        _REFS[key] = R.Reference(params, X, Y, cfg, weights=MR.mask_of(MR.train_lengths(sl, ql), cfg['max_len']))
    ref = _REFS[key]
    for k, v in params.items():
        np.testing.assert_array_equal(v, ref.params[k])
    return ref


def xcd_bx3_is_as_expected(model, cfg, B):
    """hidden 512 with > 64 rows runs the bf16-split XCD-local recurrence (k_lstm_*_xcd16), every other shape the fp32 one"""
    forced = os.environ.get('FSMG_XCD_BX3')
    assert bool(model.debug_read('xcd_bx3', 1)[0]) == (cfg['hidden_size'] == 512 and (B > 64 if forced is None else forced == '1'))


def check_masked(label, ref, got, ln, cfg):
    """the exact zeros first -- counted and printed per tensor (the last table of COMPONENTWISE.md's masked section) --, then
    check_all: every bound, every S == 0 element, every zero slice"""
    T = cfg['max_len']
    masked = (MR.mask_of(ln, T) == 0).reshape(ln.size, T)
    for (fam, layer), g in sorted(got.items(), key=lambda kv: (R.FAMILIES.index(kv[0][0]), -1 if kv[0][1] is None else kv[0][1])):
        if fam in R.COMPONENTWISE:
            zero = R.scale_of(ref.full, fam, layer) == 0
        elif fam == 'dz':
            zero = np.broadcast_to(masked[:, :, None, None], g.shape)
            # the reference's own rows there are zeros, so the slice-wise check holds them to 1e-30; this holds them to 0.0
            assert np.all(ref.t[(fam, layer)][zero] == 0)
        else:
            continue
        print('CWZ|%s|%s|%s|%d|%d|%d' % (label, fam, '' if layer is None else layer, int(zero.sum()), zero.size, int((g[zero] != 0).sum())))
        assert np.all(g[zero] == 0), '%s %s%s: %d nonzero where nothing contributes' % (label, fam, '' if layer is None else layer,
                                                                                     int((g[zero] != 0).sum()))
    check_all(label, ref, got)


def exact_row_weights(model, ln, T):
    """k_row_weights: w[t * B + b] = t < len[b] ? fl32(1 / ((double)n_valid + 1e-12)) : 0, and the integer n_valid"""
    B = ln.size
    want = np.where(np.arange(T)[:, None] < ln[None, :], np.float32(1.0 / (float(ln.sum()) + 1e-12)), np.float32(0)).astype(np.float32)
    assert np.array_equal(model.debug_read('row_weight', T * B).reshape(T, B), want)
    assert model.debug_read('n_valid', 1)[0] == ln.sum()


def masked_pass(model, sup, qry, sl, ql):
    model.debug_set('inplace_dlogits', 0)          # keep the logits beside dlogits
    model.forward_backward_masked(sup, qry, sl, ql)
    assert model.stats()['timeouts'] == 0
    assert model.debug_read('fused_softmax', 2)[1] == 0


# ----------------------------------------------------------------------------- a. every tensor, every shape, both GEMM kinds
@pytest.mark.parametrize('shape', R.CW_SHAPES, ids=R.shape_id)
def test_every_tensor_of_a_masked_pass_element_by_element(shape, gemm_kind):
    """Beside the tensors: row_weight and n_valid exactly; the loss in tail[1] within M * e32['ce'] of the fp64 masked loss,
    relative (a sum of positive terms: its S is the loss itself); tail[0] = sum dx^2 from the bound on dx -- an element of dx errs
    by d <= M * e32 * S, its square by 2 |dx| d + d^2, the squares are formed and added in fp64 (k_sqnorm_partials) and the sum
    is rounded to fp32 once: |tail[0] - ref| <= 2 M e32 sum |dx| S + (M e32)^2 sum S^2 + 2^-24 ref (+ 1e-30)."""
    cfg, (sup, qry), (sl, ql), ln = case(shape)
    T, B = cfg['max_len'], ln.size
    if T == 96:       # the two-level embedding gradient needs its heavy tokens (test_gpu_parity.py, same episode) ...
        counts = np.bincount(np.concatenate([sup.ravel(), qry.ravel()]), minlength=cfg['input_size'])
        assert counts[0] > 900 and (counts > 48).sum() >= 4, counts[:8]
    model = new_model(cfg, max_sequences=B)
    xcd_bx3_is_as_expected(model, cfg, B)
    ref = reference(R.shape_id(shape), model, sup, qry, sl, ql, cfg)
    if T == 96:       # ... and sums the start word in two levels too, most of its terms zeros (k_token_prep_len's fixed ids)
        assert (ref.X == cfg['input_size']).sum() > 48 and (ref.X == cfg['input_size']).sum() == B + int((T - ln).sum())
    masked_pass(model, sup, qry, sl, ql)
    exact_row_weights(model, ln, T)
    label = '%s|%s' % (R.shape_id(shape), gemm_kind)
    tail = model.debug_read('tail', 16)
    loss_err = abs(float(tail[1]) - ref.loss) / ref.loss
    dx, S = ref.t[('dx', None)], ref.full['scales']['dx']
    tol = M * ref.e32['dx']
    want0 = ref.full['aux']['embedding_slices_sq']
    bound0 = 2 * tol * float((np.abs(dx) * S).sum()) + tol * tol * float((S * S).sum()) + U * want0 + R.UNDERFLOW
    err0 = abs(float(tail[0]) - want0)
    print('CWL|%s|loss %.3f x e32 (%.1e)|tail0 %.3f of its bound (%.1e relative)' % (label, loss_err / ref.e32['ce'], ref.e32['ce'],
                                                                                   err0 / bound0, bound0 / want0))
    got = device_tensors(model, cfg, B)
    check_masked(label, ref, got, ln, cfg)
    assert loss_err <= M * ref.e32['ce'], (loss_err, ref.e32['ce'])
    assert err0 <= bound0, (err0, bound0)


# ----------------------------------------------------------------------------- b. only t = 0 is scored
@pytest.mark.parametrize('shape', FAMILY_SHAPES, ids=R.shape_id)
def test_all_lengths_one_element_by_element(shape, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg, (sup, qry), (sl, ql), ln = case(shape, all_ones=True)
    T, B, H, L = cfg['max_len'], ln.size, cfg['hidden_size'], cfg['n_layers']
    model = new_model(cfg, max_sequences=B)
    xcd_bx3_is_as_expected(model, cfg, B)
    ref = reference(R.shape_id(shape) + '/ones', model, sup, qry, sl, ql, cfg)
    # what the case is about, stated of the reference so that it cannot silently degrade: h_-1 = 0 and dz = 0 from t = 1 on, so nothing
    # contributes to a recurrent weight; nothing arrives at t >= 1
    later = np.arange(B * T) % T >= 1
    for l in range(L):
        S = ref.full['scales']['kernel_%d' % l]
        assert np.all(S[-H:] == 0) and np.all(S[:-H, :2 * H] > 0) and np.all(S[:-H, 3 * H:] > 0), l
        assert np.all(ref.full['dz'][l][later] == 0) and np.all(np.abs(ref.full['dz'][l][~later]).max(axis=1) > 0)
    for name in ('dlogits', 'dh', 'dx'):
        assert np.all(ref.full['scales'][name][later] == 0) and np.all(ref.full['scales'][name][~later] > 0), name
    masked_pass(model, sup, qry, sl, ql)
    exact_row_weights(model, ln, T)
    got = device_tensors(model, cfg, B)
    for l in range(L):
        assert np.all(got[('kernel', l)][-H:] == 0), 'recurrent weights of layer %d' % l
    check_masked('ones-%s|bx3' % R.shape_id(shape), ref, got, ln, cfg)
    loss_err = abs(float(model.debug_read('tail', 16)[1]) - ref.loss) / ref.loss
    print('CWL|ones-%s|bx3|loss %.3f x e32 (%.1e)' % (R.shape_id(shape), loss_err / ref.e32['ce'], ref.e32['ce']))
    assert loss_err <= M * ref.e32['ce']


# ----------------------------------------------------------------------------- c. law 2 on the intermediates
@pytest.mark.parametrize('shape', FAMILY_SHAPES, ids=R.shape_id)
def test_padding_never_matters_in_any_tensor_of_the_pass(shape, monkeypatch):
    """tests/test_masked.py's law 2 compares gradients; here every tensor device_tensors reads -- logits, lse, ce, dlogits, dh, dx,
    hs, cs, dz of every layer and the gradients -- of two handles, the second one fed other tokens behind every song's end"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    cfg, (sup, qry), (sl, ql), ln = case(shape)
    B = ln.size
    rng = np.random.RandomState(shape[4] + 200)
    sup2, qry2 = MR.scramble_padding(sup, sl, cfg['input_size'], rng), MR.scramble_padding(qry, ql, cfg['input_size'], rng)
    assert not np.array_equal(sup, sup2) or not np.array_equal(qry, qry2)
    got = []
    for s, q in ((sup, qry), (sup2, qry2)):
        model = new_model(cfg, max_sequences=B)
        masked_pass(model, s, q, sl, ql)
        got.append(device_tensors(model, cfg, B))
        got[-1][('tail', None)] = model.debug_read('tail', 2)
        model.close()
    assert got[0].keys() == got[1].keys() and len(got[0]) == 10 + 5 * cfg['n_layers']
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


# ----------------------------------------------------------------------------- d. the fused softmax
FUSED_PATHS = {'default': {}, 'serial': {'FSMG_XCD_OVERLAP': '0'}}
_FUSED_DONE = set()


@pytest.mark.parametrize('path', sorted(FUSED_PATHS))
def test_fused_softmax_masked_gradients_element_by_element(path, monkeypatch):
    """the one path whose dlogits is never materialised (k_ce_finish_w: c = w_r / S): gradients only, the XCD-partitioned and the
    serial order against one reference"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    for k, v in FUSED_PATHS[path].items():
        monkeypatch.setenv(k, v)
    cfg, (sup, qry), (sl, ql), ln = case(FUSED)
    T, B = cfg['max_len'], ln.size
    assert MR.mask_of(ln, T).mean() >= 0.25 and ln.min() == 1 and ln.max() == T and not (ln[16:32] > T // 2).any()
    model = new_model(cfg, max_sequences=B)
    ref = reference('fused', model, sup, qry, sl, ql, cfg)
    try:
        model.forward_backward_masked(sup, qry, sl, ql)
        assert model.stats()['timeouts'] == 0
        assert list(model.debug_read('fused_softmax', 2)) == [1.0, 1.0]
        exact_row_weights(model, ln, T)
        got = device_tensors(model, cfg, B, with_intermediates=False)
        check_masked('fused-%s-%s|bx3' % (path, R.shape_id(FUSED)), ref, got, ln, cfg)
        loss_err = abs(float(model.debug_read('tail', 16)[1]) - ref.loss) / ref.loss
        print('CWL|fused-%s|bx3|loss %.3f x e32 (%.1e)' % (path, loss_err / ref.e32['ce'], ref.e32['ce']))
        assert loss_err <= M * ref.e32['ce']
    finally:
        _FUSED_DONE.add(path)
        if len(_FUSED_DONE) == len(FUSED_PATHS):         # a large reference: not kept beyond its two cases
            _REFS.pop('fused', None)


# ----------------------------------------------------------------------------- e. the masked eval, relative
def forward_ce(params, X, Y, cfg, scored):
    """forward-only restatement: -> the fp64 masked NLL, and e32['ce'] = the fp32 forward pass's error in ce's measure
    |ce32 - ce64| / (|lse| + |logit_y|) maximised over the scored rows"""
    _, c64 = O.forward(params, X, Y, cfg)
    _, c32 = O.forward({k: v.astype(np.float32) for k, v in params.items()}, X, Y, cfg)
    assert c32['ce'].dtype == np.float32
    n = X.size
    S = np.abs(c64['lse']) + np.abs(c64['logits'][np.arange(n), Y.reshape(n)])
    e32 = float((np.abs(c32['ce'].astype(np.float64) - c64['ce']) / S)[scored].max())
    return float((c64['ce'] * scored).sum() / (int(scored.sum()) + 1e-12)), e32          # (masked_ref.masked_loss's form)


def test_eval_masked_relative_to_the_fp64_value():
    """three episodes with different n_valid, one of them all length 1: each NLL within M * e32['ce'] of its fp64 value, RELATIVE
    (tests/test_masked.py holds the same calls to 1e-4 absolute, which at an NLL of ~3.6 is 35 times as wide as M * e32)"""
    cfg = small_config()
    T, N, Q = cfg['max_len'], 2, 2
    rng = np.random.RandomState(11)
    queries = rng.randint(0, cfg['input_size'], size=(3, N, Q, T)).astype(np.int32)
    lens = np.stack([MR.lengths_for(rng, (N, Q), T), np.ones((N, Q), np.int32), MR.lengths_for(rng, (N, Q), T)])
    lens[2, 0, 0] = T // 2
    assert len({int(l.sum()) for l in lens}) == 3
    model = new_model(cfg)
    params = f64_params(model)
    got = model.eval_batch_masked(queries, lens)
    assert got.shape == (3,)
    assert list(model.debug_read('n_valid', 3)) == [float(l.sum()) for l in lens]
    for e in range(3):
        X, Y = O.eval_xy(queries[e], cfg['input_size'])
        scored = MR.mask_of(lens[e].reshape(-1), T) == 1
        want, e32 = forward_ce(params, X, Y, cfg, scored)
        assert want == MR.eval_step(params, queries[e], lens[e], cfg)
        assert 1e-8 < e32 < 1e-5, e32
        one = model.eval_step_masked(queries[e], lens[e])
        print('CWE|episode %d|n_valid %d|batch %.3f x e32|single %.3f x e32|e32 %.1e' % (
            e, int(lens[e].sum()), abs(float(got[e]) - want) / want / e32, abs(one - want) / want / e32, e32))
        assert abs(float(got[e]) - want) <= M * e32 * want, (e, got[e], want)
        assert abs(one - want) <= M * e32 * want, (e, one, want)
