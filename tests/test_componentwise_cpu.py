"""The componentwise measure of tests/backward_ref.py, on the CPU alone: the restatement is the oracle, the fp32 yardstick
e32 is a number, and the measure sees planted errors that max|err| / max|ref| < 2e-4 (tests/test_gpu_parity.py) lets through.

Every planted error is applied to the fp64 reference itself, so what is tested is the measure, not a kernel.
"""
import numpy as np
import pytest

import backward_ref as R
from conftest import small_config
from gpu_utils import rel_max
from oracle import lstm_oracle as O

REL_MAX_BAR = 2e-4          # the whole-tensor bound of tests/test_gpu_parity.py
M = 8                       # the device's bound is M * e32; a planted error must miss it by a factor of 10 at least

_REFS = {}


def reference(shape):
    key = R.shape_id(shape) + '/%d' % shape[4]
    if key not in _REFS:
        over, N, K, Q, seed = shape
        cfg = small_config(**over)
        sup, qry = R.episode(cfg, N, K, Q, seed)
        X, Y = O.train_xy(sup, qry, cfg['input_size'])
        _REFS[key] = (cfg, R.Reference(O.glorot_init(cfg, 0), X, Y, cfg))
    return _REFS[key]


@pytest.mark.parametrize('layers', [1, 2])
def test_restatement_is_the_oracle_bit_for_bit(layers):
    cfg = small_config(hidden_size=20, embedding_size=10, input_size=50, max_len=7, n_layers=layers)
    sup, qry = R.episode(cfg, 2, 2, 1, 3)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    params = O.glorot_init(cfg, 1)
    _, cache = O.forward(params, X, Y, cfg)
    grads, aux = O.backward(params, cache, cfg)
    full = R.backward_full(params, cache, cfg)
    assert sorted(full['grads']) == sorted(grads)
    for k in grads:
        assert full['grads'][k].dtype == np.float64
        np.testing.assert_array_equal(full['grads'][k], grads[k])
    assert full['aux'] == aux
    # the intermediates are the ones the gradients are made of
    n = X.size
    np.testing.assert_array_equal(full['dlogits'].sum(axis=0), grads['softmax_b'])
    np.testing.assert_array_equal(full['dz'][0].sum(axis=0), grads['bias_0'])
    assert full['dh'].shape == (n, cfg['hidden_size']) and full['dx'].shape == (n, cfg['embedding_size'])
    if layers == 1:
        np.testing.assert_array_equal(full['dh'], full['dlogits'].dot(params['softmax_w'].T))
    else:
        np.testing.assert_array_equal(full['dh'], full['dz'][1].dot(params['kernel_1'][:cfg['hidden_size']].T))
    for k, S in full['scales'].items():
        assert np.all(S >= 0) and np.all(np.isfinite(S)), k


@pytest.mark.parametrize('shape', R.CW_SHAPES, ids=R.shape_id)
def test_e32_of_every_family_is_a_number(shape):
    cfg, ref = reference(shape)
    assert sorted(ref.e32) == sorted(R.FAMILIES)
    for fam, e in ref.e32.items():
        # plain fp32 arithmetic: above the unit roundoff 2^-24 = 6e-8 divided by a few, far below the old 2e-4
        assert np.isfinite(e) and 1e-8 < e < 1e-4, (fam, e)
    # the reference holds itself inside the bound it sets, every element
    for (fam, layer), ref_t in ref.t.items():
        assert not ref.failures(fam, layer, ref_t, M).any()


def _fails_by(ratio_over_e32):
    return ratio_over_e32 / M


@pytest.mark.parametrize('idx', [0, 1, 2, 3, 12])
def test_zeroed_smallest_bias_unit_is_seen(idx):
    cfg, ref = reference(R.CW_SHAPES[idx])
    g = ref.full['grads']['bias_0']
    planted = g.copy()
    planted[np.argmin(np.abs(g))] = 0.0
    assert rel_max(planted, g) < REL_MAX_BAR
    ratio, where = ref.ratio('bias', 0, planted)
    assert _fails_by(ratio) >= 10, ratio
    assert ref.failures('bias', 0, planted, M).sum() == 1


# the long Zipf episode of the two-level embedding-gradient test, twice as long: the padding token's row grows with the
# episode, a rare token's row does not -- at T = 96 the dropped occurrence still shows at 2.6e-4, here it does not
LONG = (dict(hidden_size=64, embedding_size=40, input_size=500, max_len=192), 5, 3, 3, 17)


def test_dropped_single_occurrence_of_a_rare_token_is_seen():
    cfg, ref = reference(LONG)
    g = ref.full['grads']['embedding']
    counts = np.bincount(ref.X.ravel(), minlength=cfg['input_size'] + 1)
    singles = np.nonzero(counts == 1)[0]
    assert len(singles) > 0 and counts[0] > 1800
    tok = singles[np.argmin(np.abs(g[singles]).max(axis=1))]
    planted = g.copy()
    planted[tok] = 0.0                                   # its one slice never arrived
    assert rel_max(planted, g) < REL_MAX_BAR
    ratio, where = ref.ratio('embedding', None, planted)
    assert where[0] == tok and _fails_by(ratio) >= 10, (ratio, where)


@pytest.mark.parametrize('idx', [10, 11])
def test_doubled_low_probability_column_of_dlogits_is_seen(idx):
    cfg, ref = reference(R.CW_SHAPES[idx])
    dl = ref.full['dlogits']
    r = dl.shape[0] // 2
    c = int(np.argmin(np.abs(dl[r])))
    planted = dl.copy()
    planted[r, c] *= 2.0
    assert rel_max(planted, dl) < REL_MAX_BAR
    ratio, where = ref.ratio('dlogits', None, planted)
    assert where == (r, c) and _fails_by(ratio) >= 10, (ratio, where)
    assert ref.failures('dlogits', None, planted, M).sum() == 1


def test_an_absent_tokens_row_must_be_exactly_zero():
    cfg, ref = reference(R.CW_SHAPES[2])
    g, S = ref.full['grads']['embedding'], ref.full['scales']['embedding']
    counts = np.bincount(ref.X.ravel(), minlength=cfg['input_size'] + 1)
    absent = np.nonzero(counts == 0)[0]
    assert len(absent) > 0 and np.all(S[absent] == 0) and np.all(S[counts > 0] > 0)
    assert not ref.failures('embedding', None, g, M).any()
    planted = g.copy()
    planted[absent[0], 0] = 1e-30                        # inside the underflow slack of every other element
    bad = ref.failures('embedding', None, planted, M)
    assert bad.sum() == 1 and bad[absent[0], 0]
