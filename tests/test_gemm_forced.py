"""-m gpu: the bf16-split GEMM kernels FORCED onto every GEMM of a step at the shapes where tiled kernels go wrong.

Under the default dispatch (csrc/api_schedule.hip use_h_gemm / use_ws_gemm) the 256 x 256-tile k_gemm_bx3h needs hundreds of output tiles
or K >= 2048, the merged dKx + dKh GEMM (GemmArgs::m_split) and the fused softmax ride on it, and the wave-specialised k_gemm_bx3w
takes a few measured shapes: the oracle only ever meets them at full size, where every dimension spans many tiles.  FSMG_GEMM_H,
FSMG_GEMM_WS and FSMG_MAX_SPLIT are read by fsmg_create, per handle, and fsmg_debug_read("gemm_kinds") tells which kernels a handle
launched -- so handles of ONE process can run the same seeded parameters and episode through each kernel at a single partial tile, a
tile plus a few rows / columns, N = V1p (a multiple of 4 and of nothing larger), a vocabulary that ends inside a 64-column slice,
K shorter than the software pipeline and split-K slabs at small M x N, and be held to

  * each other, bit for bit, for the same K split (same LDS image, k order and term order in every variant),
  * the fp64 oracle, with the bounds of test_gpu_parity.py::test_forced_kernel_families_on_a_reduced_shape_list,
  * the cross-entropy pass, for the fused softmax, with the bounds of test_fused_softmax_matches_the_cross_entropy_pass.

The GEMMs of a train pass as (M, N, K), with rows = B * T, Ep = round_up(E, 16), V1 = input_size + 1, V1p = round_up(V1, 4),
G4 = 4 * Hp, in_p = Ep for layer 0 and Hp above it:

  zx (rows, G4, in_p) per layer   projection (rows, V1p, Hp)   dH (rows, Hp, V1p)   dW (Hp, V1p, rows)
  dKh (Hp, G4, rows) and dKx (in_p, G4, rows) per layer -- or, where in_p % 256 == 0 and the 256-tile kernel takes it, ONE merged dK
  (in_p + Hp, G4, rows) with m_split = in_p -- and dx (rows, in_p, G4) per layer.
"""
import numpy as np
import pytest

from conftest import small_config
from gpu_utils import f64_params, new_model, read_states, rel_max
from oracle import lstm_oracle as O
from test_gpu_parity import NLL_RTOL, SHAPES, _episode, cached_oracle_step

pytestmark = pytest.mark.gpu

# (config overrides, N, K, Q, (Ep, Hp, V1p) as compute_dims gives them).  B = N * (K + Q).  Every shape keeps V1 < 8 * H * L, so no handle
# takes the two-stream order (its auxiliary lane has lds_pad != 0, which no 256-tile or wave-specialised kernel runs under).
# No K split unless stated: rows / 2 < 256 or, for the products over G4 / V1p / Hp, K / 2 < 256.
CASES = {
    # everything inside one partial tile; rows = 60, Ep = 16, Hp = 16, V1p = 40, G4 = 64
    #   zx (60, 64, 16)  projection (60, 40, 16): K = Hp = 16, ONE k tile, shorter than the pipeline  dH (60, 16, 40)  dW (16, 40, 60)
    #   dKh (16, 64, 60)  dKx (16, 64, 60)  dx (60, 16, 64)
    'one_partial_tile': (dict(), 2, 2, 1, (16, 16, 40)),
    # one full row tile plus four rows, one column into the second column tile: rows = 260 (B = 20, T = 13), V1 = 257, V1p = 260;
    # hidden 48 pads to Hp = 64 (compute_dims: the persistent recurrent kernels), G4 = 256, Ep = 32
    #   zx (260, 256, 32)  projection (260, 260, 64)  dH (260, 64, 260)  dW (64, 260, 260)  dKh (64, 256, 260)  dKx (32, 256, 260)  dx (260, 32, 256)
    'rows_260_v1_257': (dict(hidden_size=48, embedding_size=24, input_size=256, max_len=13), 5, 3, 1, (32, 64, 260)),
    # exactly one row tile and one column tile: rows = 256 (B = 16, T = 16), V1 = V1p = 256
    #   zx (256, 256, 32)  projection (256, 256, 64)  dH (256, 64, 256)  dW (64, 256, 256)  dKh (64, 256, 256)  dKx (32, 256, 256)  dx (256, 32, 256)
    'rows_256_v1_256': (dict(hidden_size=48, embedding_size=24, input_size=255, max_len=16), 4, 3, 1, (32, 64, 256)),
    # the vocabulary ends inside a 64-column slice (V1 = 301 = 256 + 45, V1p = 304): SHAPES[2], rows = 405 (B = 45, T = 9)
    #   zx (405, 256, 32)  projection (405, 304, 64)  dH (405, 64, 304)  dW (64, 304, 405)  dKh (64, 256, 405)  dKx (32, 256, 405)  dx (405, 32, 256)
    'v1_301': SHAPES[2] + ((32, 64, 304),),
    # SHAPES[20]: E = 250 pads to ONE 256-row tile, Hp = 320: rows = 270 (B = 45, T = 6), G4 = 1280, V1p = 304
    #   zx (270, 1280, 256)  projection (270, 304, 320)  dH (270, 320, 304)  dW (320, 304, 270)  dx (270, 256, 1280): S = 5 on every bf16-split
    #   kernel (K = G4 = 1280)  merged dK (576, 1280, 270) with m_split = 256: three row tiles, the last one 64 rows;
    #   where the 256-tile kernel does not run: dKh (320, 1280, 270) + dKx (256, 1280, 270)
    'hp_320_merged_dk': SHAPES[20] + ((256, 320, 304),),
    # ... with two layers: layer 1 has in_p = Hp = 320, not a multiple of 256, so dKh (320, 1280, 270) + dKx (320, 1280, 270) stay a pair
    # and zx (270, 1280, 320), dx (270, 320, 1280) of layer 1 are KC x XC / KC x KC products with partial second tiles
    'hp_320_two_layers': (dict(SHAPES[20][0], n_layers=2),) + SHAPES[20][1:] + ((256, 320, 304),),
    # split-K slabs on the 256-tile kernel at small M x N: rows = 1080 (B = 45, T = 24), Hp = 128, G4 = 512, V1 = 121, V1p = 124.
    #   pick_split(tile_mn = 256, slots = 256): t(S) = t_mfma * 256 / (tiles * S) + S * t_slab for S > 1, S <= 4 because 1080 / 5 < 256;
    #   dKh (128, 512, 1080): 2 tiles, t_mfma = 0.83 us, t_slab = 0.13 us: t = 107, 53.6, 35.9, 27.2 us for S = 1 .. 4 -> S = 4
    #   dW (128, 124, 1080): 1 tile, t_mfma = 0.20 us, t_slab = 0.03 us: t = 51.6, 25.9, 17.3, 13.0 us -> S = 4;  dKx (16, 512, 1080) never runs
    #   on the 256-tile kernel (gathered A), S = 4 on the 128-tile one by the same arithmetic
    #   zx (1080, 512, 16)  projection (1080, 124, 128)  dH (1080, 128, 124)  dx (1080, 16, 512): S = 2 (K = 512)
    'split_k_hidden_128': (dict(hidden_size=128, embedding_size=16, input_size=120, max_len=24), 5, 5, 4, (16, 128, 124)),
    # two stacked layers at hidden 64: rows = 54 (B = 9, T = 6), G4 = 256; dx of layer 1 is a KC x KC product with N = Hp
    #   zx (54, 256, 16), (54, 256, 64)  projection (54, 124, 64)  dH (54, 64, 124)  dW (64, 124, 54)  dKh (64, 256, 54) x 2
    #   dKx (16, 256, 54), (64, 256, 54)  dx (54, 16, 256), (54, 64, 256)
    'two_layers_hidden_64': (dict(hidden_size=64, embedding_size=16, input_size=120, max_len=6, n_layers=2), 3, 2, 1, (16, 64, 124)),
}
CASE_IDS = sorted(CASES)

H0_WS0 = dict(FSMG_GEMM_H='0', FSMG_GEMM_WS='0')
H0_WS2 = dict(FSMG_GEMM_H='0', FSMG_GEMM_WS='2')
H2 = dict(FSMG_GEMM_H='2')
ONE_K_RANGE = dict(FSMG_MAX_SPLIT='1', FSMG_FUSED_SOFTMAX='0')


def forced_model(monkeypatch, cfg, B, **env):
    """a handle created under `env`: the dispatch knobs are read by fsmg_create and stay with the handle"""
    with monkeypatch.context() as mp:
        for k in ('FSMG_GEMM', 'FSMG_GEMM_H', 'FSMG_GEMM_WS', 'FSMG_MAX_SPLIT', 'FSMG_FUSED_SOFTMAX', 'FSMG_MERGE_DK'):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        return new_model(cfg, max_sequences=B)


def case(name):
    over, N, K, Q, dims = CASES[name]
    cfg = small_config(**over)
    sup, qry = _episode(cfg, N, K, Q, seed=3)
    return over, cfg, N, K, Q, dims, sup, qry


def gemm_kinds(model):
    return [int(x) for x in model.debug_read('gemm_kinds', 4)]


def expected_kinds(cfg, dims, env):
    """GEMM launches of the FIRST train pass of a handle in the serial order, [fp32 MFMA, k_gemm_bx3, k_gemm_bx3w, k_gemm_bx3h], from the
    dispatch code (api_schedule.hip use_h_gemm / use_ws_gemm, api_backward.hip dk_gemm).  A pass has 3 + 4 L GEMMs: the projection, dH,
    dW and per layer zx, dKh, dKx, dx -- one fewer for every layer whose dKx + dKh are one merged GEMM."""
    Ep, Hp, V1p = dims
    L = cfg['n_layers']
    n = 3 + 4 * L
    if env.get('FSMG_GEMM') == 'f32':
        return [n, 0, 0, 0]
    if env.get('FSMG_GEMM_H') == '2':
        # wherever it can run: everything but a GEMM whose x-contiguous A is gathered and is not the first part of a merged dK -- layer
        # 0's dKx (embedding rows by token id), which then follows use_ws_gemm's default rule (XC x XC: 256 128-tiles or more; never
        # here) onto k_gemm_bx3.  Merged: in_p % 256 == 0 (api_backward.hip dk_gemm; its other conditions hold at every shape here).
        merged = [(Ep if l == 0 else Hp) % 256 == 0 for l in range(L)]
        return [0, 0 if merged[0] else 1, 0, n - sum(merged) - (0 if merged[0] else 1)]
    if env.get('FSMG_GEMM_WS') == '2':
        return [0, 0, n, 0]
    if env.get('FSMG_GEMM_WS') == '0':
        return [0, n, 0, 0]
    # the default rules at these sizes: no GEMM has the 16 / 32 / 64 / 512 256-tiles or the K >= 2048 / 4096 that use_h_gemm asks for; use_ws_gemm
    # takes the KC x KC products with K <= 4096 -- dH (K = V1p) and every layer's dx (K = G4) -- and nothing else (projection: K >= 384 and
    # 512 tiles; XC x XC: 256 tiles)
    assert V1p <= 4096 and 4 * Hp <= 4096 and Hp < 384
    return [0, n - 1 - L, 1 + L, 0]


def read_pass(model, cfg, B):
    T, V1p = cfg['max_len'], model.debug_dims()['V1p']
    out = {'logits': model.debug_read('logits', B * T * V1p).reshape(B * T, V1p)[:, :cfg['input_size'] + 1].copy(), 'lse': model.debug_read('lse', B * T), 'ce': model.debug_read('ce', B * T)}
    for k in model.param_shapes:
        out['grad ' + k] = model.get_grad(k)
    return out


@pytest.mark.parametrize('name', CASE_IDS)
def test_every_bf16_split_kernel_gives_the_same_bits_at_the_tile_edges(name, monkeypatch):
    """DESIGN.md's "same bits for the same K split" (tests/test_gemm_variants.py: one production shape) at the edge shapes: one K range per
    GEMM (FSMG_MAX_SPLIT=1) and the cross-entropy pass in every handle, then logits, lse, ce and every gradient word for word between the
    128-tile kernel, the wave-specialised one, the 256-tile one wherever it can run, and the default dispatch.  No tolerance to choose."""
    over, cfg, N, K, Q, dims, sup, qry = case(name)
    B = N * (K + Q)
    got = {}
    for label, env in (('bx3', H0_WS0), ('bx3w', H0_WS2), ('bx3h', H2), ('default', {})):
        m = forced_model(monkeypatch, cfg, B, **dict(env, **ONE_K_RANGE))
        d = m.debug_dims()
        assert (d['Ep'], d['Hp'], d['V1p']) == dims
        m.debug_set('inplace_dlogits', 0)                       # keep the logits beside dlogits
        m.forward_backward(sup, qry)
        assert gemm_kinds(m) == expected_kinds(cfg, dims, env), label
        assert list(m.debug_read('fused_softmax', 2)) == [0.0, 0.0]
        got[label] = read_pass(m, cfg, B)
        m.close()
    for label in ('bx3w', 'bx3h', 'default'):
        for k, ref in got['bx3'].items():
            np.testing.assert_array_equal(got[label][k], ref, err_msg='%s: %s' % (label, k))
    assert np.isfinite(got['bx3']['ce']).all() and (got['bx3']['ce'] > 0).all()
    m = forced_model(monkeypatch, cfg, B, FSMG_GEMM='f32', **ONE_K_RANGE)
    m.forward_backward(sup, qry)
    assert gemm_kinds(m) == expected_kinds(cfg, dims, dict(FSMG_GEMM='f32'))


def edge_slices(name, cfg, dims):
    """the part of a gradient that the LAST, partial tile of its GEMM wrote, as (label, parameter, index): a bound on the whole tensor's
    largest element would hide a wrong edge tile, because the largest element sits elsewhere"""
    Ep, Hp, V1p = dims
    E, V1 = cfg['embedding_size'], cfg['input_size'] + 1
    out = []
    if Hp == 320:
        # kernel_0 is [E + H, 4H]: on the device the x part pads to in_p = 256 rows, so rows >= 256 of the merged product (its second and
        # third row tiles) are the h rows, and its third, 64-row tile is h units 256 ..
        out += [('kernel_0 rows >= 256 of the merged dK', 'kernel_0', np.s_[E:]), ('kernel_0 last row tile', 'kernel_0', np.s_[E + 256:])]
    if V1 > 256:
        out += [('softmax_w columns >= 256', 'softmax_w', np.s_[:, 256:]), ('softmax_b columns >= 256', 'softmax_b', np.s_[256:])]
    return out


ORACLE_VARIANTS = [('bx3h+fused', H2, True), ('bx3h', dict(H2, FSMG_FUSED_SOFTMAX='0'), False), ('bx3w', H0_WS2, False)]


@pytest.mark.parametrize('variant', ORACLE_VARIANTS, ids=[v[0] for v in ORACLE_VARIANTS])
@pytest.mark.parametrize('name', CASE_IDS)
def test_forced_kernels_match_the_oracle_at_the_tile_edges(name, variant, monkeypatch):
    """Default K split.  Loss, h, c, every gradient and the squared norm of the embedding slices against the fp64 oracle, one update, then
    the evaluation of the query set (forward only: the projection's epilogue leaves softmax partials instead of logits) -- the bounds of
    test_gpu_parity.py::test_forced_kernel_families_on_a_reduced_shape_list.  At the tile-plus-a-few shapes the gradient bound also holds
    for the part the last, partial tile wrote, against that slice's own largest reference element (edge_slices)."""
    label, env, fused = variant
    over, cfg, N, K, Q, dims, sup, qry = case(name)
    B, L = N * (K + Q), cfg['n_layers']
    model = forced_model(monkeypatch, cfg, B, **env)
    params = f64_params(model)
    loss, cache, grads, aux = cached_oracle_step(('shape', repr(sorted(over.items())), N, K, Q), params, sup, qry, cfg)
    model.forward_backward(sup, qry)
    assert gemm_kinds(model) == expected_kinds(cfg, dims, env)
    assert model.debug_read('fused_softmax', 2)[1] == float(fused)       # whether the pass took it: only with dW on the 256-tile kernel
    tail = model.debug_read('tail', 16)
    print('%s %s: loss %.3e' % (name, label, abs(tail[1] - loss) / abs(loss)))
    assert abs(tail[1] - loss) <= NLL_RTOL * abs(loss)
    for l in range(L):
        hs, cs, _ = read_states(model, cfg, l, B)
        assert rel_max(hs, cache['layers'][l]['hs']) < 2e-5 and rel_max(cs, cache['layers'][l]['cs']) < 2e-5, 'layer %d' % l
    got = {k: model.get_grad(k) for k in grads}
    for k in grads:
        print('%s %s: grad %s %.3e' % (name, label, k, rel_max(got[k], grads[k])))
    for what, k, idx in edge_slices(name, cfg, dims):
        print('%s %s: %s %.3e' % (name, label, what, rel_max(got[k][idx], grads[k][idx])))
    for k in grads:
        assert rel_max(got[k], grads[k]) < 2e-4, k
    for what, k, idx in edge_slices(name, cfg, dims):
        assert rel_max(got[k][idx], grads[k][idx]) < 2e-4, what
    assert abs(tail[0] - aux['embedding_slices_sq']) <= 1e-4 * aux['embedding_slices_sq']
    opt = O.new_opt_state(params)
    O.apply_update(params, grads, aux, opt, cfg)
    assert abs(model.apply_update(1.0) - loss) <= NLL_RTOL * abs(loss)
    for k, ref in params.items():
        assert rel_max(model.get_param(k), ref) < 5e-4, k
    before = gemm_kinds(model)
    want = O.eval_step(params, qry, cfg)
    nll = model.eval_step(qry)
    assert abs(nll - want) <= NLL_RTOL * abs(want)
    # an evaluation pass is L zx GEMMs and the projection with the cross-entropy epilogue, on the forced kernel both (zx of layer 0
    # gathers K-contiguous rows, which the 256-tile kernel takes)
    assert [a - b for a, b in zip(gemm_kinds(model), before)] == ([0, 0, 0, L + 1] if env.get('FSMG_GEMM_H') == '2' else [0, 0, L + 1, 0])
    st = model.stats()
    assert st['timeouts'] == 0 and st['softmax_range_rows'] == 0


@pytest.mark.parametrize('name', CASE_IDS)
def test_fused_softmax_matches_the_cross_entropy_pass_at_small_vocabularies(name, monkeypatch):
    """The fused softmax (exp(logit) and per-slice partials from the projection's epilogue, weighted column sums in dW, row-scaled dH) at
    vocabularies of one or two column tiles -- one that ends right behind a tile, on a tile, inside a 64-column slice -- against the same
    256-tile kernels with the cross-entropy pass: the bounds of test_gpu_parity.py::test_fused_softmax_matches_the_cross_entropy_pass."""
    over, cfg, N, K, Q, dims, sup, qry = case(name)
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


def test_split_k_slabs_on_the_256_tile_kernel_at_small_shapes(monkeypatch):
    """'split_k_hidden_128': pick_split gives dW and dKh four K slabs on the 256-tile kernel (worked out beside the shape).  That the slabs
    are there shows in the bits: four partial sums added in slab order are another association of the same terms than one K range, so
    the two handles do not agree word for word.  (How close the split handle is to the truth is the oracle test's business, above.)"""
    over, cfg, N, K, Q, dims, sup, qry = case('split_k_hidden_128')
    B = N * (K + Q)
    env = dict(H2, FSMG_FUSED_SOFTMAX='0')
    split, whole = forced_model(monkeypatch, cfg, B, **env), forced_model(monkeypatch, cfg, B, FSMG_MAX_SPLIT='1', **env)
    split.forward_backward(sup, qry); whole.forward_backward(sup, qry)
    assert gemm_kinds(split) == gemm_kinds(whole) == expected_kinds(cfg, dims, H2)
    for k in ('softmax_w', 'kernel_0'):
        gs, gw = split.get_grad(k), whole.get_grad(k)
        assert not np.array_equal(gs, gw), k + ': the K split of the 256-tile kernel did not run'
