"""-m gpu: the 256 x 256-tile GEMM k_gemm_bx3h at block tiles that are partly outside M x N, one case per branch of its wave map.

csrc/gemm_edge.h gives each of the kernel's eight waves a 128 x 64 sub-tile of the block tile and says whether that sub-tile holds
anything of the result; a wave whose sub-tile holds nothing skips the fragment reads and the MFMAs of the k loop and keeps everything
else (staging, barriers, its epilogue).  With lr x lc the live extent of a tile, nlr = ceil(lr / 128), nlc = ceil(lc / 64), nl = nlr nlc:

  nl > 4            the plain map (wave >> 2, wave & 3), dead waves only skip          lc in 129 .. 192 beside full rows
  nl <= 4, nlr = 1  the plain map already has one live wave per SIMD, waves 4-7 dead   a last row tile of at most 128 rows
  nl <= 4, nlr = 2  REMAPPED: wave w takes (w & 1, 2 (w >> 2) + ((w >> 1) & 1))        a sliver of at most 128 columns beside full rows

Every output element keeps one wave, the same k order and term order: the kernels are held to each other BIT FOR BIT the way
tests/test_gemm_forced.py does it -- FSMG_GEMM_H=2 (the 256-tile kernel wherever it can run) against FSMG_GEMM_H=0, FSMG_GEMM_WS=0 (the
128-tile kernel), one K range per GEMM (FSMG_MAX_SPLIT=1), the cross-entropy pass -- so there is no tolerance to choose.  Where the K
split is the default one the two tile sizes split differently, and the fp64 oracle with that file's bounds is the reference.

The GEMMs of a train pass as (M, N, K), with rows = B * T, Ep = round_up(E, 16), V1 = input_size + 1, V1p = round_up(V1, 4), G4 = 4 * Hp:
  zx (rows, G4, Ep)   projection (rows, V1p, Hp)   dH (rows, Hp, V1p)   dW (Hp, V1p, rows)   dKh (Hp, G4, rows)   dKx (Ep, G4, rows)
  dx (rows, Ep, G4);  merged dK (Ep + Hp, G4, rows) where Ep % 256 == 0.  A tile is written (row tile, column tile): lr x lc -> nl.
"""
import numpy as np
import pytest

from conftest import small_config
from gpu_utils import f64_params, new_model, rel_max
from oracle import lstm_oracle as O
from test_gemm_forced import H0_WS0, H2, ONE_K_RANGE, expected_kinds, forced_model, gemm_kinds, read_pass
from test_gpu_parity import NLL_RTOL, SHAPES, _episode, cached_oracle_step

pytestmark = pytest.mark.gpu

# (config overrides, N, K, Q, (Ep, Hp, V1p)); hidden 48 (64 in 'v1p_416') gives Hp = 64, G4 = 256, E = 24 to Ep = 32.  Under FSMG_GEMM_H=2 every GEMM but
# layer 0's dKx (gathered embedding rows) runs on the 256-tile kernel.
CASES = {
    # rows = 260 (B = 20, T = 13), V1 = 257, V1p = 260
    #   projection (260, 260, 64): (0, 1) 256 x 4 -> nl = 2, REMAPPED;  (1, 0) 4 x 256 -> nl = 4, waves 4-7 dead;  (1, 1) 4 x 4 -> nl = 1, the corner
    #   dH (260, 64, 260): (0, 0) 256 x 64 -> nl = 2, remapped;  (1, 0) 4 x 64 -> nl = 1      dW (64, 260, 260): (0, 0) 64 x 256 -> nl = 4;  (0, 1) 64 x 4 -> nl = 1
    #   zx (260, 256, 32): (1, 0) 4 x 256 -> nl = 4      dKh (64, 256, 260): 64 x 256 -> nl = 4      dx (260, 32, 256): 256 x 32 -> nl = 2, remapped;  4 x 32 -> nl = 1
    'rows_260_v1p_260': (dict(hidden_size=48, embedding_size=24, input_size=256, max_len=13), 5, 3, 1, (32, 64, 260)),
    # rows = 384 (B = 24, T = 16): a last row tile of exactly 128 rows;  V1 = 273, V1p = 276: a sliver of 20 columns (cfg-B's 10004 = 39 * 256 + 20)
    #   projection (384, 276, 64): (0, 1) 256 x 20 -> nl = 2, remapped;  (1, 0) 128 x 256 -> nl = 4, waves 4-7 dead;  (1, 1) 128 x 20 -> nl = 1
    #   dH (384, 64, 276): 256 x 64 -> nl = 2, remapped;  128 x 64 -> nl = 1      dW (64, 276, 384): 64 x 256 -> nl = 4;  64 x 20 -> nl = 1
    #   zx (384, 256, 32): (1, 0) 128 x 256 -> nl = 4      dKh (64, 256, 384)      dx (384, 32, 256): 256 x 32 -> nl = 2, remapped;  128 x 32 -> nl = 1
    'rows_384_v1p_276': (dict(hidden_size=48, embedding_size=24, input_size=272, max_len=16), 6, 3, 1, (32, 64, 276)),
    # V1 = 353, V1p = 356 = 256 + 100: a sliver of 65 .. 128 columns, rows = 260
    #   projection (260, 356, 64): (0, 1) 256 x 100 -> nl = 4, REMAPPED (both row halves of two column slices);  (1, 1) 4 x 100 -> nl = 2, plain
    #   dW (64, 356, 260): (0, 1) 64 x 100 -> nl = 2, plain      dH (260, 64, 356): K = 356 ends inside a k tile
    'v1p_356': (dict(hidden_size=48, embedding_size=24, input_size=352, max_len=13), 5, 3, 1, (32, 64, 356)),
    # V1 = 413, V1p = 416 = 256 + 160: a sliver of 129 .. 192 columns (hidden 64 = Hp: V1 stays below 8 * H, above it a handle takes the
    # two-stream order, whose auxiliary lane no 256-tile kernel runs under)
    #   projection (260, 416, 64): (0, 1) 256 x 160 -> nl = 6: the plain map, waves 3 and 7 dead;  (1, 1) 4 x 160 -> nl = 3, plain
    #   dW (64, 416, 260): (0, 1) 64 x 160 -> nl = 3
    'v1p_416': (dict(hidden_size=64, embedding_size=24, input_size=412, max_len=13), 5, 3, 1, (32, 64, 416)),
    # SHAPES[20]: E = 250 pads to ONE 256-row tile, Hp = 320, G4 = 1280, rows = 270 (B = 45, T = 6), V1p = 304
    #   merged dK (576, 1280, 270), m_split = 256: three row tiles, the last one 64 rows: 64 x 256 -> nl = 4, waves 4-7 dead, five column tiles
    #   projection (270, 304, 320): (0, 1) 256 x 48 -> nl = 2, remapped;  (1, 1) 14 x 48 -> nl = 1      dH (270, 320, 304): (0, 1) 256 x 64 -> nl = 2, remapped
    #   dW (320, 304, 270): (1, 0) 64 x 256 -> nl = 4;  (0, 1) 256 x 48 -> nl = 2, remapped;  (1, 1) 64 x 48 -> nl = 1
    'hp_320_merged_dk': SHAPES[20] + ((256, 320, 304),),
}
CASE_IDS = sorted(CASES)
# split-K slabs with an edge tile: tests/test_gemm_forced.py 'split_k_hidden_128' -- rows = 1080 (B = 45, T = 24), Hp = 128, G4 = 512, V1p = 124;
# by pick_split's arithmetic worked out there, S = 4 for dKh (128, 512, 1080): two tiles of 128 x 256 -> nl = 4, waves 4-7 dead, and for
# dW (128, 124, 1080): one tile of 128 x 124 -> nl = 2;  projection (1080, 124, 128): five row tiles, the last one 56 x 124 -> nl = 2
SPLIT_K = (dict(hidden_size=128, embedding_size=16, input_size=120, max_len=24), 5, 5, 4, (16, 128, 124))


def case(spec):
    over, N, K, Q, dims = spec
    cfg = small_config(**over)
    sup, qry = _episode(cfg, N, K, Q, seed=3)
    return over, cfg, N, K, Q, dims, sup, qry


@pytest.mark.parametrize('name', CASE_IDS)
def test_edge_tiles_give_the_128_tile_kernels_bits(name, monkeypatch):
    """One K range per GEMM and the cross-entropy pass in both handles: logits, lse, ce and every gradient word for word between the
    256-tile kernel wherever it can run and the 128-tile kernel."""
    over, cfg, N, K, Q, dims, sup, qry = case(CASES[name])
    B = N * (K + Q)
    got = {}
    for label, env in (('bx3', H0_WS0), ('bx3h', H2)):
        m = forced_model(monkeypatch, cfg, B, **dict(env, **ONE_K_RANGE))
        d = m.debug_dims()
        assert (d['Ep'], d['Hp'], d['V1p']) == dims
        m.debug_set('inplace_dlogits', 0)                       # keep the logits beside dlogits
        m.forward_backward(sup, qry)
        assert gemm_kinds(m) == expected_kinds(cfg, dims, env), label
        assert list(m.debug_read('fused_softmax', 2)) == [0.0, 0.0]
        got[label] = read_pass(m, cfg, B)
        assert m.stats()['timeouts'] == 0
        m.close()
    for k, ref in got['bx3'].items():
        np.testing.assert_array_equal(got['bx3h'][k], ref, err_msg=k)
    assert np.isfinite(got['bx3']['ce']).all() and (got['bx3']['ce'] > 0).all()
    assert all(np.abs(v).max() > 0 for k, v in got['bx3'].items() if k.startswith('grad '))


def test_split_k_slabs_with_edge_tiles_match_the_oracle(monkeypatch):
    """The default K split (four slabs for dW and dKh, each slab an edge tile): the 128-tile kernel splits these products differently, so the
    reference is the fp64 oracle with the bounds of tests/test_gemm_forced.py::test_forced_kernels_match_the_oracle_at_the_tile_edges --
    with and without the fused softmax."""
    over, cfg, N, K, Q, dims, sup, qry = case(SPLIT_K)
    B = N * (K + Q)
    whole = forced_model(monkeypatch, cfg, B, FSMG_MAX_SPLIT='1', FSMG_FUSED_SOFTMAX='0', **H2)
    whole.forward_backward(sup, qry)
    for label, env in (('fused', H2), ('cross-entropy pass', dict(H2, FSMG_FUSED_SOFTMAX='0'))):
        model = forced_model(monkeypatch, cfg, B, **env)
        assert (model.debug_dims()['Ep'], model.debug_dims()['Hp'], model.debug_dims()['V1p']) == dims
        params = f64_params(model)
        loss, cache, grads, aux = cached_oracle_step(('shape', repr(sorted(over.items())), N, K, Q), params, sup, qry, cfg)
        model.forward_backward(sup, qry)
        assert gemm_kinds(model) == expected_kinds(cfg, dims, H2), label
        tail = model.debug_read('tail', 16)
        assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss), label
        for k in grads:
            print('%s: grad %s %.3e' % (label, k, rel_max(model.get_grad(k), grads[k])))
            assert rel_max(model.get_grad(k), grads[k]) < 2e-4, (label, k)
        for k in ('softmax_w', 'kernel_0') if label != 'fused' else ():      # the slabs were really there: another association of the same terms
            assert not np.array_equal(model.get_grad(k), whole.get_grad(k)), k + ': the K split of the 256-tile kernel did not run'
        assert model.stats()['timeouts'] == 0 and model.stats()['softmax_range_rows'] == 0


@pytest.mark.parametrize('name', ['rows_384_v1p_276', 'v1p_356'])
def test_fused_softmax_at_a_vocabulary_that_ends_inside_a_slice(name, monkeypatch):
    """The fused softmax leaves one partial per row and 64-column slice, also for slices of a tile that hold no live column -- k_ce_finish
    adds all 2 * ceil(V1p / 128) slots of a row, whichever wave wrote them.  V1p = 276 ends inside the FIRST slice of the second column tile
    (slot 2 live, slot 3 written by a dead wave), V1p = 356 inside the SECOND (slots 2 and 3 live, both written by remapped waves).  Against
    the same kernels with the cross-entropy pass: the bounds of test_gpu_parity.py::test_fused_softmax_matches_the_cross_entropy_pass."""
    over, cfg, N, K, Q, dims, sup, qry = case(CASES[name])
    B, T = N * (K + Q), cfg['max_len']
    a, b = forced_model(monkeypatch, cfg, B, **H2), forced_model(monkeypatch, cfg, B, FSMG_FUSED_SOFTMAX='0', **H2)
    a.forward_backward(sup, qry); b.forward_backward(sup, qry)
    assert list(a.debug_read('fused_softmax', 2)) == [1.0, 1.0] and list(b.debug_read('fused_softmax', 2)) == [0.0, 0.0]
    assert gemm_kinds(a) == gemm_kinds(b) == expected_kinds(cfg, dims, H2)
    np.testing.assert_allclose(a.debug_read('lse', B * T), b.debug_read('lse', B * T), rtol=1e-6)
    np.testing.assert_allclose(a.debug_read('ce', B * T), b.debug_read('ce', B * T), rtol=1e-5, atol=1e-6)
    for k in a.param_shapes:
        ga, gb = a.get_grad(k), b.get_grad(k)
        print('%s: grad %s %.3e' % (name, k, np.abs(ga - gb).max() / np.abs(gb).max()))
        assert np.abs(ga - gb).max() <= 2e-5 * np.abs(gb).max(), k
    la, lb = a.apply_update(1.0), b.apply_update(1.0)
    assert abs(la - lb) <= 2e-6 * abs(lb)
    assert a.stats()['softmax_range_rows'] == 0 and a.stats()['timeouts'] == 0


def test_work_queue_with_a_half_row_tile_and_a_column_sliver(monkeypatch):
    """The work-queue launches (FSMG_XCD_OVERLAP=1: the projection's tiles drawn beside the forward chain as their rows arrive, dW's beside
    the BPTT chain) at hidden 512, T = 32, 44 sequences, V1 = 2833: rows = 1408 = five full row tiles and one of 128 rows (the LAST items
    of the queue, waves 4-7 dead), V1p = 2836 = eleven column tiles and a sliver of 20 columns (remapped; corner 128 x 20 -> nl = 1);
    dW (512, 2836, 1408) has the sliver in both of its row tiles.  Against the serial order on the same kernels (FSMG_GEMM_H=2), as
    test_gpu_parity.py::test_xcd_partitioned_schedule_gives_the_same_bits compares them: the forward pair alone gives identical losses and
    gradients, with the backward pair only dW's K split differs.  No time-out, and the order was really taken."""
    over, N, K, Q = dict(input_size=2832, max_len=32, embedding_size=16, hidden_size=512, n_layers=1), 4, 7, 4
    cfg = small_config(**over)
    eps = O.synthetic_episodes(3, N, K, Q, cfg['max_len'], cfg['input_size'], seed=29)
    out = []
    monkeypatch.setenv('FSMG_XCD_BX3', '1')
    monkeypatch.setenv('FSMG_GEMM_H', '2')
    for xov, parts in (('0', '3'), ('1', '1'), ('1', '3')):
        monkeypatch.setenv('FSMG_XCD_OVERLAP', xov)
        monkeypatch.setenv('FSMG_XOV_PARTS', parts)
        model = new_model(cfg, max_sequences=N * (K + Q))
        d = model.debug_dims()
        assert (d['Hp'], d['V1p']) == (512, 2836)
        losses = [model.train_step(s_, q_) for s_, q_ in eps]
        model.forward_backward(*eps[0])
        assert int(model.debug_read('xcd_partitioned', 3)[2]) == int(xov), 'the last pass did not take the order it was asked for'
        out.append((losses, {k: model.get_grad(k) for k in model.param_shapes}, model.stats()))
        model.close()
    assert out[0][0] == out[1][0]
    assert out[2][0][0] == out[0][0][0]                           # first call, forward pass: the same bits
    for k in out[0][1]:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k])
        # (three updates with a dW that differs in its last bits: every tensor of the fourth pass may differ in ITS last bits)
        np.testing.assert_allclose(out[2][1][k], out[0][1][k], rtol=0, atol=1e-5 * np.abs(out[0][1][k]).max())
    np.testing.assert_allclose(out[2][0], out[0][0], rtol=1e-6)
    assert all(st['timeouts'] == 0 for _, _, st in out) and all(st['xcd_launches'] > 0 for _, _, st in out)


def test_validation_epilogue_at_a_corner_tile(monkeypatch):
    """Forward only: the projection's epilogue leaves softmax partials and the target logit instead of logits.  V1p = 260 and four
    episodes of five query songs, 20 sequences = 260 rows in one pass: the projection (260, 260, 64) with its sliver, its four-row tile and
    the corner.  The 256-tile handle's eval_batch equals the 128-tile handle's, bit for bit."""
    over, cfg, N, K, Q, dims, sup, qry = case(CASES['rows_260_v1p_260'])
    B = N * (K + Q)
    queries = np.stack([qry] + [_episode(cfg, N, K, Q, seed=seed)[1] for seed in (4, 5, 6)])
    got = {}
    for label, env in (('bx3', H0_WS0), ('bx3h', H2)):
        m = forced_model(monkeypatch, cfg, B, **env)
        before = gemm_kinds(m)
        got[label] = m.eval_batch(queries)
        took = [a - b for a, b in zip(gemm_kinds(m), before)]
        assert took[3 if label == 'bx3h' else 1] > 0 and sum(took) == took[3 if label == 'bx3h' else 1], (label, took)
        assert m.stats()['timeouts'] == 0
        m.close()
    assert np.isfinite(got['bx3']).all() and (got['bx3'] > 0).all()
    np.testing.assert_array_equal(got['bx3h'], got['bx3'])
