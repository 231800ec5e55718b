"""-m gpu: the store epilogue of the bf16-split GEMM kernels (csrc/gemm.hip store_tile_at) with the BIAS as the whole answer.

The edge tests (test_gemm_forced.py, test_gemm_edge_waves.py) hold the 128-tile and the 256-tile kernels to each other, and both share
this epilogue: a bias taken from the wrong column would pass them.  Here every weight in front of a bias is zero, so what a GEMM stores IS
its bias, column by column:

  softmax_w = 0, softmax_b[c] = ((37 c) mod 509 - 254) / 64: exact in fp32, distinct for every c < 509 -- in particular at columns 64, 128
  and 256 apart, the strides of a wave slice, a 128-column tile and a 256-column tile -- and at least 1/64 from every other column's;
  embedding = 0, kernel_0 = 0, bias_0 by the same rule: the x-part GEMM of layer 0 stores its bias, the recurrent product adds zeros.

Shapes (tests/test_gemm_edge_waves.py CASES, the smallest that reach every branch): 'rows_260_v1p_260' -- rows = 260 = 256 + 4 = 2 x 128 + 4,
V1 = 257, V1p = 260: a four-column sliver, three pad columns with ce_nvocab < N, a four-row tile whose passes are mostly masked -- and
'v1p_356', where the vocabulary ends inside a 64-column slice.  Both kernel families: FSMG_GEMM_H=0 FSMG_GEMM_WS=0 (k_gemm_bx3) and
FSMG_GEMM_H=2 (k_gemm_bx3h).  A handle takes the fused softmax where dW runs on the 256-tile kernel, which FSMG_GEMM_H=0 rules out; the
PROJECTION may then still be a 128-tile kernel -- under the default rules (api_schedule.hip use_h_gemm) dW needs K = rows >= 2048 and 16
256-tiles, the projection 512 of them -- so the fused-softmax store of k_gemm_bx3 and k_gemm_bx3w has a shape of its own below: hidden 512,
rows = 2048, V1 = 1801.

Bounds: bit-equality where the result is the bias itself; lse, ce at the 1e-5 of test_gpu_parity.py; exp(b) element by element within the
2e-5 the project holds logits to (fp32 exp of |x| < 4: a few 1e-7); evaluation at NLL_RTOL; gates, h, c against fp64 at the existing 2e-5.
"""
import numpy as np
import pytest

from gpu_utils import f64_params, read_states, rel_max, time_major
from oracle import lstm_oracle as O
from conftest import small_config
from test_gemm_edge_waves import CASES, case
from test_gemm_forced import H0_WS0, H2, ONE_K_RANGE, expected_kinds, forced_model, gemm_kinds
from test_gpu_parity import NLL_RTOL, _episode

pytestmark = pytest.mark.gpu

NAMES = ['rows_260_v1p_260', 'v1p_356']
FAMILIES = [('bx3', H0_WS0), ('bx3h', H2)]


def bias_rule(n):
    c = np.arange(n, dtype=np.int64)
    return (((37 * c) % 509 - 254) / 64.0).astype(np.float32)


def bias_only_model(monkeypatch, cfg, B, env):
    """a handle whose projection and x-part GEMM store nothing but their bias; -> (model, its parameters in fp64)"""
    m = forced_model(monkeypatch, cfg, B, **env)
    p = m.get_params()
    for k in ('softmax_w', 'embedding', 'kernel_0'):
        p[k] = np.zeros_like(p[k])
    p['softmax_b'] = bias_rule(p['softmax_b'].size).reshape(p['softmax_b'].shape)
    p['bias_0'] = bias_rule(p['bias_0'].size).reshape(p['bias_0'].shape)
    m.set_params(p)
    return m, f64_params(m)


def test_the_bias_rule_tells_columns_apart():
    b = bias_rule(509).astype(np.float64)
    assert len(set(b)) == 509 and np.array_equal(b * 64, np.round(b * 64))
    for d in (64, 128, 256):
        assert np.abs(b[d:] - b[:-d]).min() >= 1.0 / 64


@pytest.mark.parametrize('family', FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize('name', NAMES)
def test_cross_entropy_pass_stores_the_bias(name, family, monkeypatch):
    """Plain store with bias (the projection, nt_store): logits[r][c] == b[c] bit for bit for every row and c < V1; lse and ce against fp64."""
    label, env = family
    over, cfg, N, K, Q, dims, sup, qry = case(CASES[name])
    B, T, V1 = N * (K + Q), cfg['max_len'], cfg['input_size'] + 1
    m, params = bias_only_model(monkeypatch, cfg, B, dict(env, **ONE_K_RANGE))
    m.debug_set('inplace_dlogits', 0)
    m.forward_backward(sup, qry)
    assert gemm_kinds(m) == expected_kinds(cfg, dims, env)
    assert list(m.debug_read('fused_softmax', 2)) == [0.0, 0.0]
    V1p = m.debug_dims()['V1p']
    logits = m.debug_read('logits', B * T * V1p).reshape(B * T, V1p)
    b = bias_rule(V1)
    np.testing.assert_array_equal(logits[:, :V1], np.broadcast_to(b, (B * T, V1)))
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    b64 = b.astype(np.float64)
    lse = np.log(np.exp(b64).sum())
    ce = time_major(lse - b64[Y.reshape(-1)], B, T)
    print('%s %s: lse %.3e ce %.3e' % (name, label, rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)), rel_max(m.debug_read('ce', B * T), ce)))
    assert rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)) < 1e-5
    assert rel_max(m.debug_read('ce', B * T), ce) < 1e-5
    assert m.stats()['timeouts'] == 0


@pytest.mark.parametrize('name', NAMES)
def test_fused_softmax_stores_exp_of_the_bias(name, monkeypatch):
    """Fused-softmax store (256-tile family): E[r][c] against exp(b[c]) in fp64 element by element -- a neighbouring column's bias is at
    least 1/64 away in the exponent --, all but the one element per row that k_ce_finish patches (c == y_r); pad columns exactly 0."""
    over, cfg, N, K, Q, dims, sup, qry = case(CASES[name])
    B, T, V1 = N * (K + Q), cfg['max_len'], cfg['input_size'] + 1
    m, params = bias_only_model(monkeypatch, cfg, B, H2)
    m.forward_backward(sup, qry)
    assert gemm_kinds(m) == expected_kinds(cfg, dims, H2)
    assert list(m.debug_read('fused_softmax', 2)) == [1.0, 1.0]
    V1p = m.debug_dims()['V1p']
    E = m.debug_read('logits', B * T * V1p).reshape(B * T, V1p).astype(np.float64)
    b64 = bias_rule(V1).astype(np.float64)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    y = time_major(Y.reshape(-1), B, T)
    keep = np.ones((B * T, V1), bool)
    keep[np.arange(B * T), y] = False                            # exactly one per row, nothing else
    assert (~keep).sum(axis=1).tolist() == [1] * (B * T)
    want = np.broadcast_to(np.exp(b64), (B * T, V1))
    err = np.abs(E[:, :V1] - want) / want
    print('%s: E %.3e' % (name, err[keep].max()))
    assert err[keep].max() < 2e-5
    assert V1p > V1 and np.all(E[:, V1:] == 0)
    lse = np.log(np.exp(b64).sum())
    ce = lse - b64[y]
    print('%s: lse %.3e ce %.3e' % (name, rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)), rel_max(m.debug_read('ce', B * T), ce)))
    assert rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)) < 1e-5
    assert rel_max(m.debug_read('ce', B * T), ce) < 1e-5
    st = m.stats()
    assert st['timeouts'] == 0 and st['softmax_range_rows'] == 0


# fused-softmax store on the 128-tile kernels, default FSMG_GEMM_H: hidden 512 (Hp = 512, G4 = 2048), E = 16, B = 64 (at most 64: the serial
# order, no work queue), T = 32: rows = 2048; V1 = 1801 = 28 * 64 + 9 ends inside a slice, V1p = 1804 < 8 * H (no two-stream order).
#   dW (512, 1804, 2048): K = 2048, 2 x 8 = 16 256-tiles -> k_gemm_bx3h, so the pass takes the fused softmax;  dKh (512, 2048, 2048): the same
#   projection (2048, 1804, 512): 64 256-tiles < 512 -> a 128-tile kernel: k_gemm_bx3w under FSMG_GEMM_WS=2, k_gemm_bx3 under FSMG_GEMM_WS=0
#   zx (2048, 2048, 16), dH (2048, 512, 1804: K < 4096), dKx (16, 2048, 2048: gathered A), dx (2048, 16, 2048): the same 128-tile kernel
SERIAL = dict(FSMG_XCD_OVERLAP='0')                             # the projection from a plain launch, not from the work queue (256-tile only)
FUSED_128 = [('bx3', dict(SERIAL, FSMG_GEMM_WS='0'), [0, 5, 0, 2]), ('bx3w', dict(SERIAL, FSMG_GEMM_WS='2'), [0, 0, 5, 2])]


@pytest.mark.parametrize('family', FUSED_128, ids=[f[0] for f in FUSED_128])
def test_fused_softmax_store_of_the_128_tile_kernels(family, monkeypatch):
    """The checks of test_fused_softmax_stores_exp_of_the_bias with the projection on k_gemm_bx3 / k_gemm_bx3w.  (The bias rule repeats
    every 509 columns; at 64, 128 and 256 columns apart it still differs by at least 1/64.)"""
    label, env, kinds = family
    cfg = small_config(hidden_size=512, embedding_size=16, input_size=1800, max_len=32)
    N, K, Q = 8, 7, 1
    sup, qry = _episode(cfg, N, K, Q, seed=3)
    B, T, V1 = N * (K + Q), cfg['max_len'], cfg['input_size'] + 1
    m, params = bias_only_model(monkeypatch, cfg, B, env)
    m.forward_backward(sup, qry)
    print('%s: gemm_kinds %s fused_softmax %s' % (label, gemm_kinds(m), list(m.debug_read('fused_softmax', 2))))
    assert gemm_kinds(m) == kinds
    assert list(m.debug_read('fused_softmax', 2)) == [1.0, 1.0]
    V1p = m.debug_dims()['V1p']
    assert (m.debug_dims()['Hp'], V1p) == (512, 1804)
    E = m.debug_read('logits', B * T * V1p).reshape(B * T, V1p).astype(np.float64)
    b64 = bias_rule(V1).astype(np.float64)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    y = time_major(Y.reshape(-1), B, T)
    keep = np.ones((B * T, V1), bool)
    keep[np.arange(B * T), y] = False
    want = np.broadcast_to(np.exp(b64), (B * T, V1))
    err = np.abs(E[:, :V1] - want) / want
    lse = np.log(np.exp(b64).sum())
    ce = lse - b64[y]
    print('%s: E %.3e lse %.3e ce %.3e' % (label, err[keep].max(), rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)), rel_max(m.debug_read('ce', B * T), ce)))
    assert err[keep].max() < 2e-5
    assert V1p > V1 and np.all(E[:, V1:] == 0)
    assert rel_max(m.debug_read('lse', B * T), np.full(B * T, lse)) < 1e-5
    assert rel_max(m.debug_read('ce', B * T), ce) < 1e-5
    st = m.stats()
    assert st['timeouts'] == 0 and st['softmax_range_rows'] == 0


@pytest.mark.parametrize('family', FAMILIES, ids=[f[0] for f in FAMILIES])
@pytest.mark.parametrize('name', NAMES)
def test_forward_only_epilogue_and_x_part_bias(name, family, monkeypatch):
    """Forward only, four episodes of five query songs = 20 sequences = 260 rows in one pass.  The projection's epilogue leaves softmax partials
    and the target logit: eval_batch against the fp64 value at NLL_RTOL.  The x-part GEMM of layer 0 stores bias_0: gates0, h0 and c0 of every
    row equal row 0's bit for bit (all-zero weights, one bias; the gates at every time step too), and match fp64 within 2e-5."""
    label, env = family
    over, cfg, N, K, Q, dims, sup, qry = case(CASES[name])
    B = N * (K + Q)
    queries = np.stack([qry] + [_episode(cfg, N, K, Q, seed=seed)[1] for seed in (4, 5, 6)])
    assert queries.shape[0] * N * Q == B
    m, params = bias_only_model(monkeypatch, cfg, B, env)
    before = gemm_kinds(m)
    got = m.eval_batch(queries)
    took = [a - b for a, b in zip(gemm_kinds(m), before)]
    assert took == ([0, 0, 0, 2] if label == 'bx3h' else [0, 2, 0, 0]), took          # zx of layer 0 and the projection, on the forced kernel both
    want = np.array([O.eval_step(params, q, cfg) for q in queries])
    print('%s %s: nll %.3e' % (name, label, np.abs(got - want).max() / np.abs(want).max()))
    assert np.all(np.abs(got - want) <= NLL_RTOL * np.abs(want))
    hs, cs, gates = read_states(m, cfg, 0, B)
    np.testing.assert_array_equal(gates, np.broadcast_to(gates[:1, :, :1], gates.shape))
    np.testing.assert_array_equal(hs, np.broadcast_to(hs[:, :1], hs.shape))
    np.testing.assert_array_equal(cs, np.broadcast_to(cs[:, :1], cs.shape))
    X, Y = O.eval_xy(queries.reshape((-1,) + queries.shape[2:]), cfg['input_size'])
    _, cache = O.forward(params, X, Y, cfg)
    lay = cache['layers'][0]
    assert rel_max(gates, lay['gates']) < 2e-5 and rel_max(hs, lay['hs']) < 2e-5 and rel_max(cs, lay['cs']) < 2e-5
    assert m.stats()['timeouts'] == 0
