"""-m gpu: the train step against the fp64 oracle ELEMENT BY ELEMENT (tests/backward_ref.py has the measure).

tests/test_gpu_parity.py holds every tensor to max|err| / max|ref|, which is blind wherever a tensor's magnitude is uneven --
and the gradients span four to five decades inside one tensor (a rare token's embedding row beside the padding token's, a
low-probability vocabulary column of dlogits, the smallest unit of a bias gradient).  Here:

  * every tensor that is a sum of products is held to |got - ref| <= M * e32 * S + 1e-30 in every element, S = the sum of the
    products' magnitudes from the fp64 oracle; an element with S == 0 (an absent token's embedding row) must be exactly 0.0;
  * hs, cs and dz (the recursion has no product form) to max|err| <= M * e32 * max|ref| + 1e-30 per smallest natural slice:
    one (t, b) row of H units, for dz one gate block of it;
  * e32 is computed at run time, per shape and family: the fp32 restatement of the oracle against the fp64 oracle in the
    same measure, maximised over the family.  It comes from the reference alone.  M = 8 (the precedent of
    tests/test_cache.py) for every family and both GEMM arithmetics; the measured err / (S * e32) of
    every shape, GEMM kind and family is recorded in tests/COMPONENTWISE.md.

The intermediates of the backward pass are read through fsmg_debug_read: dlogits, dh (after a full pass dH is the input of
layer 0's chain: api_backward.hip dhout_chunk writes dlogits W^T there, dx_gemm of a layer above 0 overwrites it with
dz_l Kx_l^T, and every BPTT kernel takes it as `const float* dH`), dx, and dz, which every BPTT kernel family stores over the
activated gates it has just read, at the same addresses (lstm_step.hip k_lstm_bwd_step `gp[0] = di; gp[4] = dj; ...`, the
chain / reduce-scatter kernels likewise; lstm_xcd.hip and lstm_pair16.h `gp[0] = di; gp[4] = dj; gp[8] = df; gp[12] = dg`) --
the packed [unit block][gate][unit % 4] column order that gpu_utils.read_states undoes, and the only one the family-agnostic
weight-gradient GEMM of api_backward.hip (dk_gemm: `m.B = h->Z[l]; m.ldb = G4`) could contract with.  So dz is compared for
every family.

The parameters after the inner SGD step of the MAML-style pass are read through fsmg_debug_set("keep_adapted", 1) /
fsmg_debug_read("adapted:<name>") (fsmg_maml_forward_backward restores theta before it returns, api_step.hip; the knob keeps a
copy of theta' first): k_sgd_update and the query pass at theta' have their elementwise checks in
tests/test_gpu_maml_componentwise.py, which takes M, device_tensors and check_all from here.
"""
import os

import numpy as np
import pytest

import backward_ref as R
from conftest import small_config
from gpu_utils import f64_params, new_model, read_states, time_major
from oracle import lstm_oracle as O

pytestmark = pytest.mark.gpu

# The device's bound is M * e32.  Measured over CW_SHAPES, both GEMM kinds (tests/COMPONENTWISE.md): the worst family reaches
# 3.6 x e32, the bf16-split products of FSMG_GEMM=bx3 and the bf16-split XCD-local recurrence included -- so no family and no
# arithmetic needs another M than the one the fp32 restatement's own spread suggests.
M = 8


@pytest.fixture(params=['bx3', 'f32'])
def gemm_kind(request, monkeypatch):
    monkeypatch.setenv('FSMG_GEMM', request.param)
    return request.param


_REFS = {}


def reference(key, model, sup, qry, cfg):
    """fp64 oracle + fp32 restatement of one shape: computed once, shared by the GEMM kinds (same seeded parameters, same
    episode -- asserted), never written to"""
    params = f64_params(model)
    X, Y = O.train_xy(sup, qry, cfg['input_size'])
    if key is None:            # a case of its own, and a large one: not kept
        return R.Reference(params, X, Y, cfg)
    if key not in _REFS:
        _REFS[key] = R.Reference(params, X, Y, cfg)
    ref = _REFS[key]
    for k, v in params.items():
        np.testing.assert_array_equal(v, ref.params[k])
    return ref


def oracle_rows(a, B, T):
    """device row order t*B + b -> oracle row order b*T + t (time_major the other way round)"""
    return time_major(a, T, B)


def device_tensors(model, cfg, B, with_intermediates=True):
    """every checked tensor of the last train pass, by (family, layer), in the oracle's layout; pads cut off -- and asserted
    to be exact zeros where the code guarantees that"""
    d = model.debug_dims()
    T, H, E, L, V1 = cfg['max_len'], cfg['hidden_size'], cfg['embedding_size'], cfg['n_layers'], cfg['input_size'] + 1
    Hp, Ep, V1p = d['Hp'], d['Ep'], d['V1p']
    n = B * T
    t = {}
    for name in model.param_shapes:
        fam, _, layer = name.partition('_')
        key = (fam, int(layer)) if fam in ('kernel', 'bias') else (name, None)
        t[key] = model.get_grad(name)
    if not with_intermediates:
        return t
    for l in range(L):
        hs, cs, dz = read_states(model, cfg, l, B)              # (asserts the pad units of h and c to be exact zeros)
        t[('hs', l)], t[('cs', l)] = hs, cs
        t[('dz', l)] = np.transpose(dz, (2, 0, 1, 3))           # [T, gate, B, H] -> [B, T, gate, H]
    logits = model.debug_read('logits', n * V1p).reshape(n, V1p)
    t[('logits', None)] = oracle_rows(logits[:, :V1], B, T)
    t[('lse', None)] = oracle_rows(model.debug_read('lse', n), B, T)
    t[('ce', None)] = oracle_rows(model.debug_read('ce', n), B, T)
    assert model.debug_read('fused_softmax', 2)[1] == 0          # dlogits was materialised by the cross-entropy pass
    dlogits = model.debug_read('dlogits', n * V1p).reshape(n, V1p)
    # pad columns: elementwise.hip k_ce_rows writes `(v + i < n_vocab) ? ... : 0.0f`; ce_row_reg loads -INFINITY there, exp gives 0
    assert np.all(dlogits[:, V1:] == 0), 'pad columns of dlogits'
    t[('dlogits', None)] = oracle_rows(dlogits[:, :V1], B, T)
    # pad units of dh / pad columns of dx: products with pad rows of softmax_w / Kx, which are exact zeros (DESIGN.md section 3,
    # api_layout.hip "reference-layout host tensor -> internal padded segment (zero padded)")
    dh = model.debug_read('dh', n * Hp).reshape(n, Hp)
    assert np.all(dh[:, H:] == 0), 'pad units of dh'
    t[('dh', None)] = oracle_rows(dh[:, :H], B, T)
    dx = model.debug_read('dx', n * Ep).reshape(n, Ep)
    assert np.all(dx[:, E:] == 0), 'pad columns of dx'
    t[('dx', None)] = oracle_rows(dx[:, :E], B, T)
    return t


def check_all(label, ref, got):
    """prints err / (S * e32) of every tensor (the rows of tests/COMPONENTWISE.md), then asserts every bound"""
    failed = []
    for (fam, layer) in sorted(got, key=lambda k: (R.FAMILIES.index(k[0]), -1 if k[1] is None else k[1])):
        g = got[(fam, layer)]
        assert g.shape == ref.t[(fam, layer)].shape, (fam, layer, g.shape)
        ratio, where = ref.ratio(fam, layer, g)
        bad = ref.failures(fam, layer, g, M)
        print('CW|%s|%s|%s|%.2f|%.1e|%d|%s|%d/%d' % (label, fam, '' if layer is None else layer, ratio, ref.e32[fam], M,
                                                  tuple(int(i) for i in where), int(bad.sum()), bad.size))
        if bad.any():
            failed.append('%s%s: %d of %d outside M = %d (worst %.1f x e32 = %.1e at %s)'
                          % (fam, '' if layer is None else '_%d' % layer, int(bad.sum()), bad.size, M, ratio, ref.e32[fam], where))
    assert not failed, '%s: %s' % (label, '; '.join(failed))


@pytest.mark.parametrize('shape', R.CW_SHAPES, ids=R.shape_id)
def test_every_tensor_of_the_pass_element_by_element(shape, gemm_kind):
    over, N, K, Q, seed = shape
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    B = N * (K + Q)
    if cfg['max_len'] == 96:       # the two-level embedding gradient needs its heavy tokens (test_gpu_parity.py, same episode)
        counts = np.bincount(np.concatenate([sup.ravel(), qry.ravel()]), minlength=cfg['input_size'])
        assert counts[0] > 900 and (counts > 48).sum() >= 4, counts[:8]
    model = new_model(cfg, max_sequences=B)
    # hidden 512 with > 64 rows runs the bf16-split XCD-local recurrence (k_lstm_*_xcd16), every other shape the fp32 one
    forced = os.environ.get('FSMG_XCD_BX3')
    assert bool(model.debug_read('xcd_bx3', 1)[0]) == (cfg['hidden_size'] == 512 and (B > 64 if forced is None else forced == '1'))
    ref = reference(R.shape_id(shape), model, sup, qry, cfg)
    model.debug_set('inplace_dlogits', 0)          # keep the logits beside dlogits
    model.forward_backward(sup, qry)
    assert model.stats()['timeouts'] == 0
    got = device_tensors(model, cfg, B)
    check_all('%s|%s' % (R.shape_id(shape), gemm_kind), ref, got)


# cfg-B at full width; dW takes the 256 x 256-tile kernel from K = T * B >= 2048 rows on (api_schedule.hip use_h_gemm), B = 45:
# max_len 46 is the smallest that selects it (max_len 16 does not)
FUSED = (dict(input_size=10000, max_len=46, embedding_size=250, hidden_size=512, n_layers=1), 5, 5, 4, 3)


def test_fused_softmax_gradients_element_by_element(monkeypatch):
    """the one path whose dlogits is never materialised: gradients only"""
    monkeypatch.setenv('FSMG_GEMM', 'bx3')
    over, N, K, Q, seed = FUSED
    cfg = small_config(**over)
    sup, qry = R.episode(cfg, N, K, Q, seed)
    B = N * (K + Q)
    model = new_model(cfg, max_sequences=B)
    ref = reference(None, model, sup, qry, cfg)
    model.forward_backward(sup, qry)
    assert list(model.debug_read('fused_softmax', 2)) == [1.0, 1.0]
    got = device_tensors(model, cfg, B, with_intermediates=False)
    check_all('fused-%s|bx3' % R.shape_id(FUSED), ref, got)


# ----------------------------------------------------------------------------- the update, from the device's own gradient
U = 2.0 ** -24
F32 = np.float32


def adam_reference(g, m, v, scale):
    """the moment lines of k_adam_update (elementwise.hip) in fp64 on fp32 inputs, with the kernel's fp32 constants and its fp32
    clip scale -> (m, v, |b1 m| + |(1 - b1) g scale|)"""
    b1, b2 = float(F32(0.9)), float(F32(0.999))
    c1, c2 = float(F32(1.0) - F32(0.9)), float(F32(1.0) - F32(0.999))
    g, m, v = (np.asarray(a, np.float64) for a in (g, m, v))
    gc = g * scale
    m_new = b1 * m + c1 * gc
    v_new = b2 * v + c2 * gc * gc
    return m_new, v_new, np.abs(b1 * m) + np.abs(c1 * gc)


def adam_scalars(model, cfg, mode, grads, step):
    """scale and alpha as tid 0 of k_adam_update derives them (fp64, rounded to fp32), from the device's own gradients"""
    tail = model.debug_read('tail', 16)
    sq = sum(float((g.astype(np.float64) ** 2).sum()) for k, g in grads.items() if not (k == 'embedding' and mode == 'tf1_slices'))
    if mode == 'tf1_slices':
        sq += float(tail[0])
    gnorm = np.sqrt(sq)
    clip = float(F32(cfg['max_grad_norm']))
    scale = float(F32(clip / max(gnorm, clip)))
    lr_s = float(F32(cfg['lr'])) * 0.5 ** (step / float(F32(cfg['n_decay'])))
    t = step + 1.0
    alpha = float(F32(lr_s * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)))
    return gnorm, scale, alpha


@pytest.mark.parametrize('max_grad_norm', [0.3, 5])
@pytest.mark.parametrize('mode', ['tf1_slices', 'dense'])
@pytest.mark.parametrize('idx', [1, 3])
def test_adam_update_element_by_element(idx, mode, max_grad_norm):
    """m, v and the parameters after fsmg_apply_update against k_adam_update's arithmetic redone in fp64 from the DEVICE's
    gradient, over every element of every tensor (the first and last element of each segment of the flat buffer included),
    two steps (the second one exercises b1 * m and b2 * v).  The arithmetic is a handful of fp32 operations per element, so
    the tolerances are derived, not measured:
      m          16 * 2^-24 relative -- in the measure of this file: relative to |b1 m| + |(1 - b1) g scale|, which IS |m| in
                 the first step and wherever the two terms agree in sign; where they cancel no fp32 sum is accurate relative
                 to its result (printed: the worst error relative to |m| itself)
      v          32 * 2^-24 relative (both terms are positive)
      parameter  |delta| * 64 * 2^-24 + |p| * 2 * 2^-24, delta = alpha m / (sqrt(v) + eps) from the device's own new m and v,
                 which the two checks before have just tied to the gradient
    each plus 1e-30 for fp32 underflow."""
    over, N, K, Q, seed = R.CW_SHAPES[idx]
    cfg = small_config(**dict(over, max_grad_norm=max_grad_norm))
    model = new_model(cfg, max_sequences=N * (K + Q), clip_norm_mode=mode)
    for step in range(2):
        sup, qry = R.episode(cfg, N, K, Q, seed + step)
        model.forward_backward(sup, qry)
        grads = {k: model.get_grad(k) for k in model.param_shapes}
        before = {k: (model.get_opt_state(k), model.get_param(k)) for k in model.param_shapes}
        gnorm, scale, alpha = adam_scalars(model, cfg, mode, grads, step)
        assert model.step == step
        model.apply_update(1.0)
        assert model.step == step + 1
        got_gnorm = float(model.debug_read('gnorm', 1)[0])
        assert abs(got_gnorm - gnorm) <= 2 * U * gnorm
        assert (gnorm > max_grad_norm) == (max_grad_norm == 0.3), gnorm          # clip active / inactive as the case says
        assert (scale < 1.0) == (max_grad_norm == 0.3)
        for k in model.param_shapes:
            (m0, v0), p0 = before[k]
            m1, v1 = model.get_opt_state(k)
            p1 = model.get_param(k).astype(np.float64)
            m_ref, v_ref, m_scale = adam_reference(grads[k], m0, v0, scale)
            m_err, v_err = np.abs(m1 - m_ref), np.abs(v1 - v_ref)
            nz = m_ref != 0
            print('ADAM|%s|%s|%s|step %d|%s|m %.2f u of S, %.1f u of |m||v %.2f u|' % (
                R.shape_id(R.CW_SHAPES[idx]), mode, max_grad_norm, step, k, (m_err / np.maximum(m_scale, 1e-300)).max() / U,
                (m_err[nz] / np.abs(m_ref[nz])).max() / U if nz.any() else 0.0, (v_err / np.maximum(v_ref, 1e-300)).max() / U), end='')
            assert np.all(m_err <= 16 * U * m_scale + R.UNDERFLOW), k
            if step == 0:
                assert np.all(m_err <= 16 * U * np.abs(m_ref) + R.UNDERFLOW), k
            assert np.all(v_err <= 32 * U * v_ref + R.UNDERFLOW), k
            delta = alpha * m1.astype(np.float64) / (np.sqrt(v1.astype(np.float64)) + float(F32(1e-8)))
            p_ref = p0.astype(np.float64) - delta
            p_err = np.abs(p1 - p_ref)
            p_tol = np.abs(delta) * 64 * U + np.abs(p_ref) * 2 * U + R.UNDERFLOW
            print('p %.3f of its bound' % (p_err / p_tol).max())
            assert np.all(p_err <= p_tol), k
            if step == 0:                                  # nothing moves without a gradient (an absent token's embedding row)
                assert np.all(p1[grads[k] == 0] == p0[grads[k] == 0]), k
